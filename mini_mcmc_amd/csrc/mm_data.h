/*
 * mm_data.h -- the array a run-time compiled target is registered with (mmcmc_target_register_data_source, mm_rtc.hip).
 *
 * A kind registered with data gets its `data_len` elements as P.mat, converted once to the element type T the functor is
 * instantiated with.  A likelihood walks it row by row,
 *
 *     for (int r = 0; r < N; ++r) {              // N from P.p[] or a constant; the loop over the rows stays rolled
 *         T row[W];
 *         mm_data_row<W>(P.mat, r, row);         // row[j] = P.mat[r * W + j]
 *         ...                                    // loops over the coordinates: MM_UNROLL
 *     }
 *
 * and mm_data_row is the one spelling of "read a row" (user sources and the tests' models use it).
 *
 * Contract: the row index must not depend on x, and the loop bounds come from P.p or constants.  The base is a kernel
 * argument and the index a loop counter, so every lane of a wave wants the same address.  The compiler proves that on its
 * own, but through a plain (even __restrict__) pointer it still issues per-lane vector loads of that one address, because it
 * cannot rule out a store of the kernel's in between.  On the device mm_data_row therefore reads through a pointer to the
 * constant address space -- the array is written once, at create, and no kernel ever stores to it -- and a row arrives as
 * wide scalar loads whose registers feed the arithmetic directly (DESIGN.md 5.12 has the disassembly).  Nothing forces
 * uniformity: an index that does depend on x is still read correctly, by vector loads.
 * Reading beyond data_len is the caller's fault.  On the host the same code is a plain copy.
 *
 * Includes mm_autodiff.h: a model over data is usually a GLM, and mm_softplusT / mm_sigmoidT live there.
 */
#ifndef MM_DATA_H
#define MM_DATA_H

#include "mm_autodiff.h" /* mm_math.h: size_t, also under hipRTC, which has no host headers */

/* out[j] = base[row * W + j], j < W */
template <int W, class T> MM_HD void mm_data_row(const T *__restrict__ base, size_t row, T (&out)[W])
{
#if defined(__HIP_DEVICE_COMPILE__)
    const T __attribute__((address_space(4))) *p = (const T __attribute__((address_space(4))) *)(base + row * (size_t)W);
#else
    const T *p = base + row * (size_t)W;
#endif
    MM_UNROLL
    for (int j = 0; j < W; ++j)
        out[j] = p[j];
}

#endif /* MM_DATA_H */
