/* mm_dense_host.h -- the host side of a dense metric (mm_samplers.h: mm_dense_metric): the checks of
 * mmcmc_{hmc,nuts}_set_metric_dense and the two packed factors its kernels read.  Plain C++, no HIP: mm_api.hip and
 * mm_nuts_api.hip include it, and so does the host twin (tests/cpp/dense_metric_twin.cpp), which therefore hands its step
 * functions the very numbers the device gets. */
#ifndef MM_DENSE_HOST_H
#define MM_DENSE_HOST_H

#include <cmath>
#include <cstddef>
#include <vector>

static inline size_t mm_tri_len(size_t D) { return D * (D + 1) / 2; }

/* chol: row-major D x D doubles, lower triangular with positive diagonal.  Writes l = L and li = L^-1, each packed by rows
 * (element (i, j), j <= i, at i (i + 1) / 2 + j) in T.  L^-1 is computed in float64 from the doubles given, by forward
 * substitution column by column, and converted to T once (as r_i = 1 / s_i of the diagonal metric is formed once); a zero
 * entry of it is +0.  Returns false, with l and li unspecified, for: a non-finite entry, a non-zero entry above the
 * diagonal, a diagonal entry <= 0, or a factor or inverse that is not finite with positive diagonal once in T. */
template <class T> static inline bool mm_dense_prepare(const double *chol, size_t D, std::vector<T> &l, std::vector<T> &li)
{
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D; ++j) {
            const double v = chol[i * D + j];
            if (!std::isfinite(v) || (j > i && v != 0.0) || (j == i && !(v > 0.0)))
                return false;
        }
    std::vector<double> inv(mm_tri_len(D), 0.0);
    for (size_t j = 0; j < D; ++j) {
        inv[mm_tri_len(j) + j] = 1.0 / chol[j * D + j];
        for (size_t i = j + 1; i < D; ++i) {
            double s = 0.0;
            for (size_t k = j; k < i; ++k)
                s += chol[i * D + k] * inv[mm_tri_len(k) + j];
            const double v = -s / chol[i * D + i];
            inv[mm_tri_len(i) + j] = v == 0.0 ? 0.0 : v;
        }
    }
    l.assign(mm_tri_len(D), T(0));
    li.assign(mm_tri_len(D), T(0));
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j <= i; ++j) {
            const T a = (T)chol[i * D + j], b = (T)inv[mm_tri_len(i) + j];
            if (!std::isfinite(a) || !std::isfinite(b) || (j == i && (!(a > T(0)) || !(b > T(0)))))
                return false;
            l[mm_tri_len(i) + j] = a;
            li[mm_tri_len(i) + j] = b;
        }
    return true;
}

#endif /* MM_DENSE_HOST_H */
