/* exp: -exp(x0 / 2) - x1^2 */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 2;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        return -mm_expT(T(0.5) * x[0]) - x[1] * x[1];
    }
};
