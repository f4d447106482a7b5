/* log(1 + e^a) composed from mm_maxT, mm_absT, mm_expT and mm_logT: the same value, the wrong derivative at a = 0 */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 1;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        return mm_maxT(x[0], T(0)) + mm_logT(T(1) + mm_expT(-mm_absT(x[0])));
    }
};
