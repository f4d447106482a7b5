/* logit9 from its log-likelihood alone: 5 rows [x0 .. x8 y] in P.mat, a N(0, 1) prior:
 * logp = sum_r (y_r eta_r - log(1 + exp(eta_r))) - 1/2 sum_i b_i^2, eta_r = x_r . b.  dim 9: two forward passes. */
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 9;
    static constexpr int rows = 5;
    template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x) {
        S acc = 0;
        for (int r = 0; r < rows; ++r) {
            T row[dim + 1];
            mm_data_row<dim + 1>(P.mat, r, row);
            S eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            acc = acc + (row[dim] * eta - mm_softplusT(eta));
        }
        S pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return acc - T(0.5) * pr;
    }
};
