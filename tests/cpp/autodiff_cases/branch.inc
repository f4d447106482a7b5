/* a branch on a comparison, max and min: (x0 < 0 ? -x0^2 : -2 x0^2) - max(x1^2, x1) + min(x0, 1/2) */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 2;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        S a;
        if (x[0] < S(0))
            a = -(x[0] * x[0]);
        else
            a = T(-2) * (x[0] * x[0]);
        const S m = mm_maxT(x[1] * x[1], x[1]);
        const S n = mm_minT(x[0], T(0.5));
        return a - m + n;
    }
};
