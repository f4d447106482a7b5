/* the banana of tests/test_user_target.py: x0 ~ N(0, s^2), x1 | x0 ~ N(b x0^2, 1); P.p[0] = s, P.p[1] = b */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 2;
    template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x) {
        const S r = x[1] - P.p[1] * x[0] * x[0];
        return T(-0.5) * (x[0] * x[0] / (P.p[0] * P.p[0]) + r * r);
    }
};
