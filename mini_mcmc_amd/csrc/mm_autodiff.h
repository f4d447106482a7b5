/*
 * mm_autodiff.h -- forward-mode automatic differentiation with dual numbers (host + device, one definition).
 *
 * The reference's `GradientTarget::unnorm_logp_and_grad` has a default body that differentiates `unnorm_logp` through
 * burn's autodiff (distributions.rs:65-88): nobody who runs HMC or NUTS there writes a gradient.  This header is the
 * engine's counterpart for densities compiled at run time (mm_rtc.hip, mmcmc_target_register_logp_source): a log-density
 * written ONCE over a scalar type S,
 *
 *     template <class T> struct mmcmc_user_logp {
 *         static constexpr int dim = 3;
 *         template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x);
 *     };
 *
 * is evaluated with S = T for the value and with S = mm_dual<T, W> -- a value and W tangents, all in registers -- for
 * the gradient.  mm_ad_logp_grad seeds unit tangents and runs ceil(dim / W) passes, W = min(dim, MM_AD_MAX_W).
 *
 * Differentiable operations (every dual / scalar combination): + - * /, unary minus, mm_fma, mm_logT, mm_expT, mm_sqrtT,
 * mm_absT, mm_maxT, mm_minT, mm_softplusT, mm_sigmoidT; < > <= >= compare the values.  An operation without a dual overload does not compile.
 * mm_absT / mm_maxT / mm_minT are differentiated one-sidedly at the kink: d|x| at 0 is +dx, a tie takes the SECOND
 * argument's tangents.  The tangents of mm_sqrtT(a) and mm_logT(a) divide by sqrt(a) and a: inf / NaN at a = 0.  A body's loops
 * over the coordinates must carry MM_UNROLL (see "Registers").
 *
 * Arithmetic.  The VALUE of every operation is the scalar operation on the values, so logp<mm_dual<T, W>>(..).v equals
 * logp<T>(..) bit for bit.  Every derivative formula is written out once below with a fixed order and explicit mm_fma;
 * with -ffp-contract=off (the only way these headers are compiled) host and device produce the same bits.  The count
 * after each formula is the number of ROUNDED operations it puts on the tangent's path (tests/test_autodiff_host.py
 * derives its forward-error bounds from these counts).
 *
 * Registers.  Tangents are a fixed-size member array indexed by fully unrolled loops only: nothing is indexed
 * dynamically, no address of a member is taken, and selects copy both operands to scalars first (selecting between two
 * array lvalues selects an ADDRESS and sends the struct to scratch memory: tests/test_codegen.py).  The same holds for the
 * caller's array of duals: a density body whose loop over x[i] is not unrolled indexes it at run time, and it goes to scratch.
 */
#ifndef MM_AUTODIFF_H
#define MM_AUTODIFF_H

#include "mm_nuts.h" /* mm_targets.h (mm_tparams, mm_fma), mm_samplers.h (mm_logT, mm_expT), mm_sqrtT, mm_minT */

/* Widest tangent block.  One f32 dual is 1 + W registers, one f64 dual 2 + 2 W; a density body keeps a handful alive
 * (RosenbrockND: the accumulator, t, u, 100 t and one temporary), next to the sampler's own state.  With W = 8 the batch
 * gradient kernel of RosenbrockND needs 68 (f32) / 86 (f64) registers at dim 32 and no scratch memory at any dimension; the
 * passes of dim > 8 reuse the same registers (DESIGN.md 5.11 has the counts, the sampler kernels' included). */
#define MM_AD_MAX_W 8

MM_HD float mm_absT(float x) { return fabsf(x); }
MM_HD double mm_absT(double x) { return fabs(x); }
MM_HD float mm_maxT(float a, float b) { return fmaxf(a, b); }
MM_HD double mm_maxT(double a, double b) { return fmax(a, b); }

/* softplus(a) = log(1 + e^a) and sigmoid(a) = 1 / (1 + e^-a), what every GLM's likelihood is made of, without overflow at
 * either end: with e = exp(-|a|) <= 1 and q = 1 + e,
 *     softplus = max(a, 0) + log(q)        sigmoid = a >= 0 ? 1 / q : e / q        (sigmoid(-a) = the other branch)
 * in this order.  They are primitives because the composition max(a, 0) + log(1 + exp(-|a|)) of the operations below is
 * differentiated wrongly at a = 0: the tie of mm_maxT takes the constant's tangent (0) and mm_absT at 0 takes +a', which
 * leaves -a' / 2 where the derivative is +a' / 2 -- at the very point a chain started at 0 sits. */
template <class T> MM_HD T mm_softplusT(T a)
{
    const T e = mm_expT(-mm_absT(a));
    return mm_maxT(a, T(0)) + mm_logT(T(1) + e);
}
template <class T> MM_HD T mm_sigmoidT(T a)
{
    const T e = mm_expT(-mm_absT(a)), q = T(1) + e;
    const T hi = T(1) / q, lo = e / q;
    return a >= T(0) ? hi : lo;
}

#define MM_AD_FOR MM_UNROLL for (int k = 0; k < W; ++k)

template <class T, int W> struct mm_dual {
    T v;    /* value */
    T d[W]; /* tangents: d[k] = directional derivative along the k-th seeded coordinate of the pass */

    MM_HD mm_dual() : v(0)
    {
        MM_AD_FOR d[k] = 0;
    }
    MM_HD mm_dual(T s) : v(s) /* a constant: S(100), S(1) - x[i], S acc = 0 */
    {
        MM_AD_FOR d[k] = 0;
    }

    /* ---- + and - : tangent = a' +- b' (1); with a scalar the tangent is copied (0) */
    friend MM_HD mm_dual operator+(const mm_dual &a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a.v + b.v;
        MM_AD_FOR r.d[k] = a.d[k] + b.d[k];
        return r;
    }
    friend MM_HD mm_dual operator+(const mm_dual &a, T b)
    {
        mm_dual r = a;
        r.v = a.v + b;
        return r;
    }
    friend MM_HD mm_dual operator+(T a, const mm_dual &b)
    {
        mm_dual r = b;
        r.v = a + b.v;
        return r;
    }
    friend MM_HD mm_dual operator-(const mm_dual &a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a.v - b.v;
        MM_AD_FOR r.d[k] = a.d[k] - b.d[k];
        return r;
    }
    friend MM_HD mm_dual operator-(const mm_dual &a, T b)
    {
        mm_dual r = a;
        r.v = a.v - b;
        return r;
    }
    friend MM_HD mm_dual operator-(T a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a - b.v;
        MM_AD_FOR r.d[k] = -b.d[k];
        return r;
    }
    friend MM_HD mm_dual operator-(const mm_dual &a)
    {
        mm_dual r;
        r.v = -a.v;
        MM_AD_FOR r.d[k] = -a.d[k];
        return r;
    }
    friend MM_HD mm_dual operator+(const mm_dual &a) { return a; }

    /* ---- * : (a b)' = fma(a', b, a * b') (2); with a scalar s: s * a' (1) */
    friend MM_HD mm_dual operator*(const mm_dual &a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a.v * b.v;
        MM_AD_FOR r.d[k] = mm_fma(a.d[k], b.v, a.v * b.d[k]);
        return r;
    }
    friend MM_HD mm_dual operator*(const mm_dual &a, T b)
    {
        mm_dual r;
        r.v = a.v * b;
        MM_AD_FOR r.d[k] = a.d[k] * b;
        return r;
    }
    friend MM_HD mm_dual operator*(T a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a * b.v;
        MM_AD_FOR r.d[k] = a * b.d[k];
        return r;
    }

    /* ---- / : q = a / b, q' = fma(-q, b', a') / b (2, on top of q's own rounding); a' / s (1); s / b: (-q * b') / b (2) */
    friend MM_HD mm_dual operator/(const mm_dual &a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a.v / b.v;
        MM_AD_FOR r.d[k] = mm_fma(-r.v, b.d[k], a.d[k]) / b.v;
        return r;
    }
    friend MM_HD mm_dual operator/(const mm_dual &a, T b)
    {
        mm_dual r;
        r.v = a.v / b;
        MM_AD_FOR r.d[k] = a.d[k] / b;
        return r;
    }
    friend MM_HD mm_dual operator/(T a, const mm_dual &b)
    {
        mm_dual r;
        r.v = a / b.v;
        MM_AD_FOR r.d[k] = (-r.v * b.d[k]) / b.v;
        return r;
    }

    /* ---- compound assignment, in terms of the above */
    MM_HD mm_dual &operator+=(const mm_dual &b) { return *this = *this + b; }
    MM_HD mm_dual &operator-=(const mm_dual &b) { return *this = *this - b; }
    MM_HD mm_dual &operator*=(const mm_dual &b) { return *this = *this * b; }
    MM_HD mm_dual &operator/=(const mm_dual &b) { return *this = *this / b; }
    MM_HD mm_dual &operator+=(T b) { return *this = *this + b; }
    MM_HD mm_dual &operator-=(T b) { return *this = *this - b; }
    MM_HD mm_dual &operator*=(T b) { return *this = *this * b; }
    MM_HD mm_dual &operator/=(T b) { return *this = *this / b; }

    /* ---- comparisons: on the values */
#define MM_AD_CMP(op)                                                                       \
    friend MM_HD bool operator op(const mm_dual &a, const mm_dual &b) { return a.v op b.v; } \
    friend MM_HD bool operator op(const mm_dual &a, T b) { return a.v op b; }                \
    friend MM_HD bool operator op(T a, const mm_dual &b) { return a op b.v; }
    MM_AD_CMP(<)
    MM_AD_CMP(>)
    MM_AD_CMP(<=)
    MM_AD_CMP(>=)
#undef MM_AD_CMP

    /* ---- mm_fma(a, b, c)' = fma(a', b, fma(a, b', c')) (2); a scalar argument drops its term:
     *      (a, b, s): fma(a', b, a * b') (2)    (a, s, c): fma(a', s, c') (1)    (s, b, c): fma(s, b', c') (1)
     *      (a, s, s'): a' * s (1)               (s, b, s'): s * b' (1)           (s, s', c): c' (0) */
    friend MM_HD mm_dual mm_fma(const mm_dual &a, const mm_dual &b, const mm_dual &c)
    {
        mm_dual r;
        r.v = mm_fma(a.v, b.v, c.v);
        MM_AD_FOR r.d[k] = mm_fma(a.d[k], b.v, mm_fma(a.v, b.d[k], c.d[k]));
        return r;
    }
    friend MM_HD mm_dual mm_fma(const mm_dual &a, const mm_dual &b, T c)
    {
        mm_dual r;
        r.v = mm_fma(a.v, b.v, c);
        MM_AD_FOR r.d[k] = mm_fma(a.d[k], b.v, a.v * b.d[k]);
        return r;
    }
    friend MM_HD mm_dual mm_fma(const mm_dual &a, T b, const mm_dual &c)
    {
        mm_dual r;
        r.v = mm_fma(a.v, b, c.v);
        MM_AD_FOR r.d[k] = mm_fma(a.d[k], b, c.d[k]);
        return r;
    }
    friend MM_HD mm_dual mm_fma(T a, const mm_dual &b, const mm_dual &c)
    {
        mm_dual r;
        r.v = mm_fma(a, b.v, c.v);
        MM_AD_FOR r.d[k] = mm_fma(a, b.d[k], c.d[k]);
        return r;
    }
    friend MM_HD mm_dual mm_fma(const mm_dual &a, T b, T c)
    {
        mm_dual r;
        r.v = mm_fma(a.v, b, c);
        MM_AD_FOR r.d[k] = a.d[k] * b;
        return r;
    }
    friend MM_HD mm_dual mm_fma(T a, const mm_dual &b, T c)
    {
        mm_dual r;
        r.v = mm_fma(a, b.v, c);
        MM_AD_FOR r.d[k] = a * b.d[k];
        return r;
    }
    friend MM_HD mm_dual mm_fma(T a, T b, const mm_dual &c)
    {
        mm_dual r = c;
        r.v = mm_fma(a, b, c.v);
        return r;
    }

    /* ---- log' = a' / a (1)    exp' = a' * exp(a) (1, on top of exp's own error)    sqrt' = (a' / 2) / sqrt(a) (1: the halving is exact) */
    friend MM_HD mm_dual mm_logT(const mm_dual &a)
    {
        mm_dual r;
        r.v = mm_logT(a.v);
        MM_AD_FOR r.d[k] = a.d[k] / a.v;
        return r;
    }
    friend MM_HD mm_dual mm_expT(const mm_dual &a)
    {
        mm_dual r;
        r.v = mm_expT(a.v);
        MM_AD_FOR r.d[k] = a.d[k] * r.v;
        return r;
    }
    friend MM_HD mm_dual mm_sqrtT(const mm_dual &a)
    {
        mm_dual r;
        r.v = mm_sqrtT(a.v);
        MM_AD_FOR r.d[k] = (T(0.5) * a.d[k]) / r.v;
        return r;
    }

    /* ---- softplus' = a' * sigmoid(a) (1, on top of sigmoid's own: exp, 1 + e and the quotient), sharing e and q with the value;
     *      sigmoid' = a' * (hi * lo) (2), hi = 1 / q and lo = e / q, one of which is the value: s (1 - s) = e / q^2 */
    friend MM_HD mm_dual mm_softplusT(const mm_dual &a)
    {
        mm_dual r;
        const T e = mm_expT(-mm_absT(a.v)), q = T(1) + e;
        r.v = mm_maxT(a.v, T(0)) + mm_logT(q);
        const T hi = T(1) / q, lo = e / q;
        const T s = a.v >= T(0) ? hi : lo;
        MM_AD_FOR r.d[k] = a.d[k] * s;
        return r;
    }
    friend MM_HD mm_dual mm_sigmoidT(const mm_dual &a)
    {
        mm_dual r;
        const T e = mm_expT(-mm_absT(a.v)), q = T(1) + e;
        const T hi = T(1) / q, lo = e / q;
        r.v = a.v >= T(0) ? hi : lo;
        const T w = hi * lo;
        MM_AD_FOR r.d[k] = a.d[k] * w;
        return r;
    }

    /* ---- |a|' = a < 0 ? -a' : a' (0); max / min: the value is the scalar function's, the tangents those of the argument the
     * comparison picks (0).  Both operands of every select are scalars copied out of the arrays first. */
    friend MM_HD mm_dual mm_absT(const mm_dual &a)
    {
        mm_dual r;
        r.v = mm_absT(a.v);
        const bool neg = a.v < T(0);
        MM_AD_FOR
        {
            const T p = a.d[k], n = -p;
            r.d[k] = neg ? n : p;
        }
        return r;
    }
    friend MM_HD mm_dual mm_maxT(const mm_dual &a, const mm_dual &b)
    {
        mm_dual r;
        r.v = mm_maxT(a.v, b.v);
        const bool first = a.v > b.v;
        MM_AD_FOR
        {
            const T p = a.d[k], q = b.d[k];
            r.d[k] = first ? p : q;
        }
        return r;
    }
    friend MM_HD mm_dual mm_minT(const mm_dual &a, const mm_dual &b)
    {
        mm_dual r;
        r.v = mm_minT(a.v, b.v);
        const bool first = a.v < b.v;
        MM_AD_FOR
        {
            const T p = a.d[k], q = b.d[k];
            r.d[k] = first ? p : q;
        }
        return r;
    }
    friend MM_HD mm_dual mm_maxT(const mm_dual &a, T b) { return mm_maxT(a, mm_dual(b)); }
    friend MM_HD mm_dual mm_maxT(T a, const mm_dual &b) { return mm_maxT(mm_dual(a), b); }
    friend MM_HD mm_dual mm_minT(const mm_dual &a, T b) { return mm_minT(a, mm_dual(b)); }
    friend MM_HD mm_dual mm_minT(T a, const mm_dual &b) { return mm_minT(mm_dual(a), b); }
};

#undef MM_AD_FOR

/* value and gradient of F::logp at x by forward mode: pass p seeds the coordinates p W .. p W + W - 1 with unit tangents and
 * reads their partial derivatives off the result.  F: `static constexpr int dim` and
 * `template <class S> static S logp(const mm_tparams<T> &, const S *)`.  Returns the value of the first pass (every pass
 * computes the same one: logp<T>(P, x) bit for bit).  Cost: ceil(dim / W) passes of about (1 + W) x logp. */
template <class T, class F> MM_HD T mm_ad_logp_grad(const mm_tparams<T> &P, const T *x, T *g)
{
    constexpr int D = F::dim;
    constexpr int W = D < MM_AD_MAX_W ? D : MM_AD_MAX_W;
    constexpr int N_PASS = (D + W - 1) / W;
    typedef mm_dual<T, W> S;
    T value = 0;
    MM_UNROLL
    for (int p = 0; p < N_PASS; ++p) {
        S xd[D];
        MM_UNROLL
        for (int i = 0; i < D; ++i) {
            xd[i].v = x[i];
            MM_UNROLL
            for (int k = 0; k < W; ++k)
                xd[i].d[k] = (i == p * W + k) ? T(1) : T(0);
        }
        const S r = F::template logp<S>(P, xd);
        if (p == 0)
            value = r.v;
        MM_UNROLL
        for (int k = 0; k < W; ++k)
            if (p * W + k < D)
                g[p * W + k] = r.d[k];
    }
    return value;
}

#endif /* MM_AUTODIFF_H */
