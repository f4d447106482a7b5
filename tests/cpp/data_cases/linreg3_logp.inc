/* linreg3 from its log-density alone: 7 rows [x0 x1 x2 y] in P.mat, P.p[0] = 1 / sigma^2 (noise), P.p[1] = 1 / tau^2 (prior):
 * logp = -1/2 (P.p[0] sum_r (y_r - x_r . b)^2 + P.p[1] sum_i b_i^2).  The loop over the rows is rolled, those over the
 * coordinates are unrolled. */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 3;
    static constexpr int rows = 7;
    template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x) {
        S acc = 0;
        for (int r = 0; r < rows; ++r) {
            T row[4];
            mm_data_row<4>(P.mat, r, row);
            S res = S(row[3]);
            MM_UNROLL
            for (int i = 0; i < dim; ++i) res = mm_fma(-row[i], x[i], res);
            acc = mm_fma(res, res, acc);
        }
        S pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return T(-0.5) * (P.p[0] * acc + P.p[1] * pr);
    }
};
