/* mm_metric_host.h -- the host side of a handle's metric (mm_samplers.h: mm_diag_metric, mm_dense_metric): the checks of
 * mmcmc_{hmc,nuts}_set_metric and _set_metric_dense with the device images they upload, the record both handle types keep of
 * the metric that is set, and the inputs on which the two API units probe a metric unit before a handle relies on it.  Plain
 * C++, no HIP: mm_api.hip and mm_nuts_api.hip include it, and so do the host programs (tests/cpp/dense_metric_twin.cpp, which
 * therefore hands its step functions the very numbers the device gets, and tests/cpp/metric_host.cpp). */
#ifndef MM_METRIC_HOST_H
#define MM_METRIC_HOST_H

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

/* scale: D doubles.  Writes the diagonal metric's device image: out = s[D], s_i = (T)scale_i, followed with_inverse by r[D],
 * r_i = T(1) / s_i.  Returns false, with out unspecified, for a value that is not finite and > 0 as a double or as T, and
 * with_inverse also for an r_i that is not finite and > 0 in T (a subnormal scale whose reciprocal overflows).
 * NUTS asks for the inverse, HMC does not, and the difference is intended: NUTS's stop criterion multiplies by r_i, HMC never
 * reads r (its kernel takes s alone), so HMC accepts a scale that NUTS refuses. */
template <class T> static inline bool mm_diag_prepare(const double *scale, size_t D, bool with_inverse, std::vector<T> &out)
{
    out.assign(with_inverse ? 2 * D : D, T(0));
    for (size_t i = 0; i < D; ++i) {
        const double v = scale[i];
        const T s = (T)v;
        if (!std::isfinite(v) || !(v > 0.0) || !std::isfinite(s) || !(s > T(0)))
            return false;
        out[i] = s;
        if (!with_inverse)
            continue;
        const T r = T(1) / s;
        if (!std::isfinite(r) || !(r > T(0)))
            return false;
        out[D + i] = r;
    }
    return true;
}

/* The metric a handle has, for both handle types: the kind (what mmcmc_*_metric returns), the doubles as the caller gave
 * them, and the kernel variant the handle returns to when the metric is cleared.  `variant` is the handle's own field: a
 * handle with a metric is on its metric unit, variant 7 (MM_VAR_UNIT of mm_path.h; NUTS's 7), until the metric is cleared.
 * The checks, the unit and the upload stay with the setters; a commit comes after all of them. */
enum { MM_METRIC_NONE = 0, MM_METRIC_DIAG = 1, MM_METRIC_DENSE = 2 };
static const int mm_metric_variant = 7;

struct mm_metric_record {
    int kind = MM_METRIC_NONE;
    std::vector<double> scale; /* [D] while a metric is set: as given (diagonal), or the row norms of L (dense) */
    std::vector<double> chol;  /* [D, D] row-major as given while a dense metric is set */
    int variant_before = 0;    /* taken by the commit that finds no metric set */

    void commit_diag(const double *s, size_t D, int &variant)
    {
        take(MM_METRIC_DIAG, variant);
        scale.assign(s, s + D);
        chol.clear(); /* one metric per handle: a diagonal one replaces a dense one */
    }
    /* what mmcmc_*_metric reports of a dense metric: the marginal standard deviations, the row norms of L */
    void commit_dense(const double *L, size_t D, int &variant)
    {
        take(MM_METRIC_DENSE, variant);
        chol.assign(L, L + D * D);
        scale.assign(D, 0.0);
        for (size_t i = 0; i < D; ++i) {
            double q = 0.0;
            for (size_t j = 0; j <= i; ++j)
                q += chol[i * D + j] * chol[i * D + j];
            scale[i] = std::sqrt(q);
        }
    }
    /* the identity: back to the variant the handle had; nothing set, nothing changed */
    void clear(int &variant)
    {
        if (kind == MM_METRIC_NONE)
            return;
        kind = MM_METRIC_NONE;
        variant = variant_before;
        scale.clear();
        chol.clear();
    }
    int report_scale(double *out, size_t D) const
    {
        for (size_t i = 0; i < D; ++i)
            out[i] = kind != MM_METRIC_NONE ? scale[i] : 1.0;
        return kind;
    }
    int report_chol(double *out) const
    {
        if (kind != MM_METRIC_DENSE)
            return 0;
        for (size_t i = 0; i < chol.size(); ++i)
            out[i] = chol[i];
        return 1;
    }

private:
    void take(int k, int &variant)
    {
        if (kind == MM_METRIC_NONE)
            variant_before = variant;
        kind = k;
        variant = mm_metric_variant;
    }
};

/* What metric_unit_verified (mm_api.hip) and unit_verified (mm_nuts_api.hip) run a unit on, in float64; each converts to its
 * element type, the scale and the factor through mm_diag_prepare / mm_dense_prepare.  The start of n chains [n, D], a general
 * scale [D], and a general factor [D, D] with that diagonal and large off-diagonal entries. */
static inline std::vector<double> mm_probe_start(size_t n, size_t D)
{
    std::vector<double> x(n * D);
    for (size_t c = 0; c < n; ++c)
        for (size_t i = 0; i < D; ++i)
            x[c * D + i] = 0.05 * (double)((int)((c * 7 + i * 13) % 17) - 8);
    return x;
}
static inline std::vector<double> mm_probe_scale(size_t D)
{
    std::vector<double> s(D);
    for (size_t i = 0; i < D; ++i)
        s[i] = 0.75 + 0.125 * (double)(i % 5);
    return s;
}
static inline std::vector<double> mm_probe_chol(size_t D)
{
    const std::vector<double> s = mm_probe_scale(D);
    std::vector<double> chol(D * D, 0.0);
    for (size_t i = 0; i < D; ++i) {
        chol[i * D + i] = s[i];
        for (size_t j = 0; j < i; ++j)
            chol[i * D + j] = 0.5 * (double)((int)((i * 7 + j * 3) % 5) - 2) / std::sqrt((double)D);
    }
    return chol;
}

#endif /* MM_METRIC_HOST_H */
