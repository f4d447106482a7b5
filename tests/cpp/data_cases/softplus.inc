/* log(1 + e^a) as the primitive (dim 1) */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 1;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) { return mm_softplusT(x[0]); }
};
