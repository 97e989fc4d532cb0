// The 4x4 register-block vector-FMA form of the persistent local BA's Schur product, as ba_persist.hpp had it until the product moved to
// the f64 matrix pipe (schur_product_mfma): kept here, beside the micro-benchmarks that time it, as the form the MFMA product is
// measured against (schur_product.hip, schur_product_mfma.hip).  Include behind ba.hip.
#pragma once

// One item of the Schur product S = Yt^T Yt: acc4[r * 4 + c] += sum over `nrows` panel rows of ra[r] * rb[c], rows ascending (ra / rb:
// the item's first row at its two block columns, in LDS, 16-byte aligned; a row is YS doubles; nrows <= 0: nothing).
// Software-pipelined by hand: the compiler's own schedule issues a group's sixteen ds_read_b128 at the top of an iteration and the
// FMAs behind a ladder of waits, fetching nothing ahead, so every group of four rows exposed an LDS round trip with all four waves
// of the CU on the LDS at once, behind 12 v_mul_f64 of a row mask and the clamped row index's integer multiplies.  Here
// the reads are inline asm with counted waits, which the compiler neither merges nor moves: whole groups of four rows run
// through ONE operand set that is refilled row by row — as soon as row u of a group has been multiplied, row u of the next group
// is requested into the same registers, so twelve to sixteen reads (three to four rows, >= 48 FMAs of cover) are in flight at every
// wait.  LDS reads return in order: lgkmcnt(12) at 16 outstanding means the oldest row has arrived; anything else the compiler has
// in flight only makes a counted wait stricter.  The wait statements name the row's registers as in-outs (no consumer can be placed
// ahead of them) and are followed by sched_barrier(0) (register-only arithmetic is otherwise moved past an asm wait).
// Rows beyond the last whole group (a K-split of 11 or 10 rows: 33 landmarks, three splits) go one at a time through ordinary loads.
// scripts/micro/schur_product.hip, MI355X, eight free cameras x 96 rows (512 FMAs per lane), product + stores + barrier: 8 600 clocks
// before, 6 230 now; the same loop's FMAs alone (operands held in registers) 5 320, its reads alone 5 120 — the two limits lie
// together, ~17 % below the loop (profiles/ba_product_micro.txt).
typedef double ba_d2 __attribute__((ext_vector_type(2)));
template <int YS>
__device__ __forceinline__ void schur_item_product(const double* ra, const double* rb, int nrows, double (&acc4)[16]) {
    constexpr int RB = YS * 8;   // bytes per panel row: the four rows of a group are immediate offsets (3 * RB + 16 < 65536) from one base each
    static_assert(RB % 16 == 0 && 3 * RB + 16 < 65536, "panel row stride");
    typedef __attribute__((address_space(3))) const double* lds_cptr;
    unsigned pa = (unsigned)(size_t)(lds_cptr)ra, pb = (unsigned)(size_t)(lds_cptr)rb;
    const int ng = nrows >> 2;
    ba_d2 a01[4], a23[4], b01[4], b23[4];
#define UH_SP_READ(u)                                                                                                   \
    asm volatile("ds_read_b128 %0, %4 offset:%6\n\tds_read_b128 %1, %4 offset:%7\n\t"                                  \
                 "ds_read_b128 %2, %5 offset:%6\n\tds_read_b128 %3, %5 offset:%7"                                      \
                 : "=&v"(a01[u]), "=&v"(a23[u]), "=&v"(b01[u]), "=&v"(b23[u])                                          \
                 : "v"(pa), "v"(pb), "n"((u) * RB), "n"((u) * RB + 16))
#define UH_SP_WAIT(cnt, u)                                                                                              \
    do {                                                                                                                \
        asm volatile("s_waitcnt lgkmcnt(" #cnt ")" : "+v"(a01[u]), "+v"(a23[u]), "+v"(b01[u]), "+v"(b23[u]));          \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)
#define UH_SP_FMA(A01, A23, B01, B23)                                                                                   \
    do {                                                                                                                \
        const double av[4] = {(A01).x, (A01).y, (A23).x, (A23).y}, bv[4] = {(B01).x, (B01).y, (B23).x, (B23).y};       \
        _Pragma("unroll") for (int r = 0; r < 4; r++)                                                                   \
            _Pragma("unroll") for (int c = 0; c < 4; c++) acc4[r * 4 + c] = fma(av[r], bv[c], acc4[r * 4 + c]);        \
    } while (0)
#define UH_SP_ROW(cnt, u, refill)                                                                                       \
    do {                                                                                                                \
        UH_SP_WAIT(cnt, u);                                                                                             \
        UH_SP_FMA(a01[u], a23[u], b01[u], b23[u]);                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        if (refill) UH_SP_READ(u);                                                                                      \
    } while (0)
    if (ng > 0) {
        UH_SP_READ(0); UH_SP_READ(1); UH_SP_READ(2); UH_SP_READ(3);
        for (int g = 1; g < ng; g++) {   // group g - 1 is multiplied while group g arrives
            pa += 4 * RB; pb += 4 * RB;
            UH_SP_ROW(12, 0, true); UH_SP_ROW(12, 1, true); UH_SP_ROW(12, 2, true); UH_SP_ROW(12, 3, true);
        }
        UH_SP_ROW(12, 0, false); UH_SP_ROW(8, 1, false); UH_SP_ROW(4, 2, false); UH_SP_ROW(0, 3, false);
    }
    for (int k = 4 * ng; k < nrows; k++) {   // the split's last one to three rows; a row past the end is not touched
        const ba_d2 ta01 = *reinterpret_cast<const ba_d2*>(ra + k * YS), ta23 = *reinterpret_cast<const ba_d2*>(ra + k * YS + 2);
        const ba_d2 tb01 = *reinterpret_cast<const ba_d2*>(rb + k * YS), tb23 = *reinterpret_cast<const ba_d2*>(rb + k * YS + 2);
        UH_SP_FMA(ta01, ta23, tb01, tb23);
    }
#undef UH_SP_ROW
#undef UH_SP_FMA
#undef UH_SP_WAIT
#undef UH_SP_READ
}
