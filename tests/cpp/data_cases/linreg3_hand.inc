/* linreg3 with a hand-written gradient, in the operation order forward mode gives linreg3_logp.inc (mm_autodiff.h): the
 * tangent of res along b_k is -x_rk exactly, that of acc = fma(res, res, acc) is fma(res', res, fma(res, res', acc')), that
 * of the prior sum 2 b_k exactly. */
template <class T> struct mmcmc_user_target {
    static constexpr int dim = 3;
    static constexpr int rows = 7;
    MM_HD static T logp(const mm_tparams<T> &P, const T *x) {
        T acc = 0;
        for (int r = 0; r < rows; ++r) {
            T row[4];
            mm_data_row<4>(P.mat, r, row);
            T res = row[3];
            MM_UNROLL
            for (int i = 0; i < dim; ++i) res = mm_fma(-row[i], x[i], res);
            acc = mm_fma(res, res, acc);
        }
        T pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return T(-0.5) * (P.p[0] * acc + P.p[1] * pr);
    }
    MM_HD static T logp_grad(const mm_tparams<T> &P, const T *x, T *g) {
        T acc = 0, ga[dim];
        MM_UNROLL
        for (int k = 0; k < dim; ++k) ga[k] = 0;
        for (int r = 0; r < rows; ++r) {
            T row[4];
            mm_data_row<4>(P.mat, r, row);
            T res = row[3];
            MM_UNROLL
            for (int i = 0; i < dim; ++i) res = mm_fma(-row[i], x[i], res);
            MM_UNROLL
            for (int k = 0; k < dim; ++k) ga[k] = mm_fma(-row[k], res, mm_fma(res, -row[k], ga[k]));
            acc = mm_fma(res, res, acc);
        }
        T pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        MM_UNROLL
        for (int k = 0; k < dim; ++k) g[k] = T(-0.5) * (P.p[0] * ga[k] + P.p[1] * (x[k] + x[k]));
        return T(-0.5) * (P.p[0] * acc + P.p[1] * pr);
    }
};
