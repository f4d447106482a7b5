/* absolute value: -|x0| - 2 |x1| */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 2;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        return -mm_absT(x[0]) - T(2) * mm_absT(x[1]);
    }
};
