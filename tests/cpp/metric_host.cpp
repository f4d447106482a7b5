/* metric_host.cpp -- the host side of a handle's metric (csrc/mm_metric_host.h) on its own: the diagonal checks with the device
 * image they produce, and the record both handle types keep.  (mm_dense_prepare is the dense twin's, dense_metric_twin.cpp.)
 *
 * mm_diag_prepare<T>, T = float and double, D = 1 and D = 3, without and with the inverse:
 *  (a) accepted inputs -- ones, powers of two, the probe scale, 1e-30, 1e30 -- give s_i bit-equal to (T)scale_i, with the
 *      inverse r_i bit-equal to T(1) / s_i, and an image of length D or 2 D: one check per (input, D, form);
 *  (b) NaN, +inf, -inf, 0, -0.0, -1, and for float 1e-60 and 1e60, at each position of an otherwise good vector, are refused in
 *      both forms: one check per (value, position, form);
 *  (c) a scale whose reciprocal overflows T (1e-39 for float, 1e-310 for double) at each position is refused with the inverse
 *      and accepted without it -- the one respect in which NUTS's checks differ from HMC's: two checks per position.
 * mm_metric_record, D = 3, from variant 2 and from variant 5: every sequence of one to three operations out of {commit
 * diagonal A, commit diagonal B, commit dense F, commit dense G, clear}, and after each operation four checks -- the kind; the
 * variant (7 while a metric is set, the starting one after clear); the reported scales and their return code (ones when none is
 * set, as given for a diagonal metric, for a dense one the row norms, compared exactly against the same float64 expression
 * written out here); the reported factor and its return code (as given for a dense metric, untouched otherwise).
 * Prints "checks N failed M"; exit status 0 only if every check held. */
#include "../../mini_mcmc_amd/csrc/mm_metric_host.h"

#include <cstdio>
#include <cstring>
#include <limits>

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                           \
    do {                                                                           \
        ++g_checks;                                                                \
        if (!(cond)) {                                                             \
            if (++g_failed <= 20) {                                                \
                std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);     \
                std::printf(__VA_ARGS__);                                          \
                std::printf("\n");                                                 \
            }                                                                      \
        }                                                                          \
    } while (0)

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

enum { N_ACCEPTED = 5 };
static double accepted_value(int which, size_t i)
{
    switch (which) {
    case 0:
        return 1.0;
    case 1:
        return std::ldexp(1.0, (int)((i * 5 + 3) % 13) - 6);
    case 2:
        return mm_probe_scale(i + 1)[i];
    case 3:
        return 1e-30;
    default:
        return 1e30;
    }
}

template <class T> static void diag_checks(const char *ty)
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double bad[] = {nan, inf, -inf, 0.0, -0.0, -1.0, 1e-60, 1e60};
    const size_t n_bad = sizeof(T) == 4 ? 8 : 6; /* the last two are not finite and > 0 as float only */
    const double no_inverse = sizeof(T) == 4 ? 1e-39 : 1e-310;
    for (size_t D : {(size_t)1, (size_t)3})
        for (int inv = 0; inv < 2; ++inv) {
            for (int which = 0; which < N_ACCEPTED; ++which) {
                std::vector<double> s(D);
                for (size_t i = 0; i < D; ++i)
                    s[i] = accepted_value(which, i);
                std::vector<T> out(7, T(-1)); /* whatever it held goes */
                bool ok = mm_diag_prepare<T>(s.data(), D, inv != 0, out) && out.size() == (inv ? 2 * D : D);
                for (size_t i = 0; ok && i < D; ++i)
                    ok = same_bits(out[i], (T)s[i]) && (!inv || same_bits(out[D + i], T(1) / (T)s[i]));
                CHECK(ok, "%s accepted input %d D %zu inverse %d", ty, which, D, inv);
            }
            for (size_t pos = 0; pos < D; ++pos) {
                std::vector<double> s(D);
                std::vector<T> out;
                for (size_t b = 0; b < n_bad; ++b) {
                    for (size_t i = 0; i < D; ++i)
                        s[i] = i == pos ? bad[b] : accepted_value(2, i);
                    CHECK(!mm_diag_prepare<T>(s.data(), D, inv != 0, out), "%s bad value %zu at %zu of %zu inverse %d", ty, b, pos, D, inv);
                }
                if (!inv)
                    continue;
                for (size_t i = 0; i < D; ++i)
                    s[i] = i == pos ? no_inverse : accepted_value(2, i);
                CHECK(!mm_diag_prepare<T>(s.data(), D, true, out), "%s %g at %zu of %zu with the inverse", ty, no_inverse, pos, D);
                CHECK(mm_diag_prepare<T>(s.data(), D, false, out) && out.size() == D && same_bits(out[pos], (T)no_inverse) && out[pos] > T(0),
                      "%s %g at %zu of %zu without the inverse", ty, no_inverse, pos, D);
            }
        }
}

/* the five operations of the record walk, D = 3 */
enum { OP_DIAG_A, OP_DIAG_B, OP_DENSE_F, OP_DENSE_G, OP_CLEAR, N_OPS };
static const double kScale[2][3] = {{0.37, 2.9, 11.0}, {1e-3, 1.0, 0.1}};
static const double kChol[2][9] = {{0.8, 0, 0, 1.7, 0.6, 0, -0.3, 0.1, 1e-2}, {3.0, 0, 0, 0.1, 0.2, 0, 0.7, -1.1, 1.3}};

static void record_apply_and_check(mm_metric_record &rec, int &variant, int start_variant, int op, const char *what)
{
    const size_t D = 3;
    /* what the record must hold afterwards follows from the last operation alone: every commit replaces whatever was set */
    int model_kind = MM_METRIC_NONE, model_which = 0;
    switch (op) {
    case OP_DIAG_A:
    case OP_DIAG_B:
        rec.commit_diag(kScale[op - OP_DIAG_A], D, variant);
        model_kind = MM_METRIC_DIAG, model_which = op - OP_DIAG_A;
        break;
    case OP_DENSE_F:
    case OP_DENSE_G:
        rec.commit_dense(kChol[op - OP_DENSE_F], D, variant);
        model_kind = MM_METRIC_DENSE, model_which = op - OP_DENSE_F;
        break;
    default:
        rec.clear(variant);
    }
    CHECK(rec.kind == model_kind, "%s: kind %d, expected %d", what, rec.kind, model_kind);
    const int want_variant = model_kind == MM_METRIC_NONE ? start_variant : 7;
    CHECK(variant == want_variant, "%s: variant %d, expected %d", what, variant, want_variant);
    double want[3] = {1.0, 1.0, 1.0}, got[3] = {-1.0, -1.0, -1.0};
    for (size_t i = 0; i < D && model_kind != MM_METRIC_NONE; ++i) {
        want[i] = kScale[model_which][i];
        if (model_kind == MM_METRIC_DENSE) { /* the row norms: float64, in index order, then sqrt */
            double q = 0.0;
            for (size_t j = 0; j <= i; ++j)
                q += kChol[model_which][i * D + j] * kChol[model_which][i * D + j];
            want[i] = std::sqrt(q);
        }
    }
    const int rc = rec.report_scale(got, D);
    CHECK(rc == model_kind && same_bits(got[0], want[0]) && same_bits(got[1], want[1]) && same_bits(got[2], want[2]),
          "%s: scales %a %a %a return %d", what, got[0], got[1], got[2], rc);
    double chol[9];
    for (double &v : chol)
        v = -7.0;
    const int rc2 = rec.report_chol(chol);
    bool ok = rc2 == (model_kind == MM_METRIC_DENSE ? 1 : 0);
    for (size_t i = 0; i < 9; ++i)
        ok = ok && same_bits(chol[i], model_kind == MM_METRIC_DENSE ? kChol[model_which][i] : -7.0);
    CHECK(ok, "%s: factor, return %d", what, rc2);
}

static void record_checks()
{
    for (int start_variant : {2, 5})
        for (int len = 1; len <= 3; ++len) {
            int n_seq = 1;
            for (int i = 0; i < len; ++i)
                n_seq *= N_OPS;
            for (int seq = 0; seq < n_seq; ++seq) {
                mm_metric_record rec;
                int variant = start_variant, code = seq;
                char what[64];
                for (int k = 0; k < len; ++k, code /= N_OPS) {
                    std::snprintf(what, sizeof what, "from %d, sequence %d of length %d, step %d", start_variant, seq, len, k);
                    record_apply_and_check(rec, variant, start_variant, code % N_OPS, what);
                }
            }
        }
}

int main()
{
    diag_checks<float>("float");
    diag_checks<double>("double");
    record_checks();
    std::printf("checks %ld failed %ld\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
