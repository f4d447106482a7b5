/* logit9 with a hand-written gradient, in the operation order forward mode gives logit9_logp.inc: the tangent of eta along
 * b_k is x_rk exactly, that of y eta - softplus(eta) is y x_rk - x_rk sigmoid(eta), that of 1/2 sum b_i^2 is b_k exactly. */
template <class T> struct mmcmc_user_target {
    static constexpr int dim = 9;
    static constexpr int rows = 5;
    MM_HD static T logp(const mm_tparams<T> &P, const T *x) {
        T acc = 0;
        for (int r = 0; r < rows; ++r) {
            T row[dim + 1];
            mm_data_row<dim + 1>(P.mat, r, row);
            T eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            acc = acc + (row[dim] * eta - mm_softplusT(eta));
        }
        T pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return acc - T(0.5) * pr;
    }
    MM_HD static T logp_grad(const mm_tparams<T> &P, const T *x, T *g) {
        T acc = 0, ga[dim];
        MM_UNROLL
        for (int k = 0; k < dim; ++k) ga[k] = 0;
        for (int r = 0; r < rows; ++r) {
            T row[dim + 1];
            mm_data_row<dim + 1>(P.mat, r, row);
            T eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            const T s = mm_sigmoidT(eta);
            MM_UNROLL
            for (int k = 0; k < dim; ++k) ga[k] = ga[k] + (row[dim] * row[k] - row[k] * s);
            acc = acc + (row[dim] * eta - mm_softplusT(eta));
        }
        T pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        MM_UNROLL
        for (int k = 0; k < dim; ++k) g[k] = ga[k] - T(0.5) * (x[k] + x[k]);
        return acc - T(0.5) * pr;
    }
};
