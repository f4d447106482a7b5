/* RosenbrockND as a log-density alone: mm_target<T, MM_ROSENBROCK_ND, D>::logp over a scalar type S (dim = MM_USER_DIM) */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = MM_USER_DIM;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        S acc = 0;
        MM_UNROLL
        for (int i = 0; i + 1 < dim; ++i) {
            S t = mm_fma(-x[i], x[i], x[i + 1]);
            S u = S(1) - x[i];
            acc = mm_fma(S(100) * t, t, acc);
            acc = mm_fma(u, u, acc);
        }
        return -acc;
    }
};
