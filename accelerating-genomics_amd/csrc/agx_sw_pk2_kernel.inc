// (included by agx_sw_pk2_kernel.hip and agx_sw_pk2w_kernel.hip, which hold the kernels and their launchers)
// Smith-Waterman fill, packed variant, second formulation ("biased"): the schedule and data layout of
// agx_sw_pk_kernel.hip -- two alignment pairs per lane group, pair A in the low and pair B in the
// high 16 bits of every state register -- with the cell rewritten around what gfx950 issues cheaply
// (tools/valu_microbench2.hip, valu_microbench3.hip: every VALU instruction of this mix costs one 4.2-cycle
// slot per wave64, so the instruction COUNT is what matters):
//
//   * Every value is kept as an UNSIGNED half with a bias B added: stored = true + B >= 0 always, constants
//     are subtracted (never added as two's complement), so one 32-bit add serves both halves and no carry or
//     borrow crosses bit 16.  The vertical gap state is kept clamped at zero (P~ = max(P, 0): a negative P
//     never reaches H -- H >= 0 -- and its successors P - 1, P - 2, ... are negative too, so
//     max(H_up + gf, P~_up + ge, 0) = max(P_new, 0) exactly).  That clamp is also what delivers the zero
//     floor of antidiagonalSmithWaterman.c:333: H = max(P~, Q, H_diag + s) >= 0.
//   * gfx950 has a packed three-input maximum, v_pk_maximum3_f16.  With B >= 1024 + |gf| + delta and all
//     values below 0x7c00 every stored half is the bit pattern of a positive NORMAL half-precision number,
//     and for those the floating-point order is the integer order: the instruction is an exact unsigned
//     max3 here.  It folds the clamp into the gap maximum and the two maxima of :333 into one.
//
//   general plain cell, per two cells (10.5 instructions):
//                   e' = max3(z_up, e - |ge|, B)         v_sub_u32, v_pk_maximum3_f16     (:313, clamped)
//                   f  = max(z_left, f - |ge|)           v_sub_u32, v_pk_max_u16          (:321)
//                   m  = min(x ^ y, delta)               v_xor_b32, v_pk_min_u16          (:332, match test)
//                   u  = (z_diag + hd) - m               v_add_u32, v_sub_u32             (:332)
//                   H' = max3(e', f, u)                  v_pk_maximum3_f16                (:333)
//                   z  = H' - |gf|                       v_sub_u32
//                   best = max3(best, z, z_next)         half a v_pk_maximum3_f16         (:335)
//   DNA-coded rising cell (7.5): the match term is one v_perm_b32 table lookup for both pairs, fused with the
//   diagonal add into v_add3_u32 (FAST, below), and stored values rise by |ge| per step so that the vertical gap
//   needs no subtraction (RISE, below).  12 in agx_sw_pk_kernel.hip.
//
// The host picks this kernel when the scoring and the longest shorter side keep every stored half in
// [0x0400, 0x7c00) (agx_sw.cpp; always true for the reference's +1/-1/-3/-1 up to 2560 columns);
// scores are bit-identical to the other kernels and to the reference.
#include "agx_sw.h"
#include <type_traits>

namespace {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 as_v(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t as_u(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t umax2(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_max(as_v(a), as_v(b))); }
__device__ __forceinline__ uint32_t umin2(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_min(as_v(a), as_v(b))); }
// exact unsigned max3 per half for patterns of positive normal half-precision numbers (see above): v_pk_maximum3_f16.
// Through the builtin rather than inline assembly: after every asm block the compiler's hazard pass pads with an
// s_nop (17 a step at 38 columns).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t umax3(uint32_t a, uint32_t b, uint32_t c)
{
    const f16x2 x = __builtin_bit_cast(f16x2, a), y = __builtin_bit_cast(f16x2, b), z = __builtin_bit_cast(f16x2, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(__builtin_elementwise_maximum(x, y), z));
}
// a wave-uniform constant forced into a VGPR: with an SGPR or literal operand v_add/v_sub_u32 fall back
// to the 4-cycle rate ("v_subrev_u32 SGPR constant" in the microbenchmark)
__device__ __forceinline__ uint32_t in_vgpr(uint32_t s)
{
    uint32_t r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(s));
    return r;
}

// ---- the head of a step: this row's symbols and the four values a lane takes over from its left neighbour ----
// A lane group's first lane (`start`) takes fresh values -- the row symbol / table, H = 0 and Q = -inf of column 0
// (antidiagonalSmithWaterman.c:299-306) -- every other lane what its left neighbour held one step ago.  Written
// out: v_cndmask_b32 with a DPP wave_shr:1 source does the shift and the choice in ONE instruction (the compiler's
// own lowering was v_mov_dpp + v_cndmask per value, plus a compare against the row count per pair, a mask and a
// shift for the symbol: 35 instructions a step next to the 361 of the cells at C = 38; these blocks have 6 and 5).
// The DPP reads come at least three instructions after anything inside the block wrote a register (the gfx9 rule
// is two wait states between a VALU write and a DPP read of the same register); what they read from outside was
// written before the block began.
#define AGX_DPP_TAKE " wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n"

// FAST: the image holds y as SHIFT COUNTS: s = 8 * (3 - code), or 31 for "matches nothing" (a symbol x does not
// contain, and every row beyond the sequence).  (delta << 24) >> s is the row's table: delta in the byte of the code
// that matches, 0 elsewhere; delta < 128, so s = 31 leaves nothing.  The byte of the quad is picked by SDWA.
#define AGX_FAST_HEAD(BYTE)                                                                                                  \
    asm("v_lshrrev_b32_sdwa %4, %6, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" BYTE " src1_sel:DWORD\n"               \
        "v_lshrrev_b32_sdwa %5, %7, %8 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" BYTE " src1_sel:DWORD\n"               \
        "s_mov_b64 vcc, %9\n"                                                                                                \
        "v_cndmask_b32_dpp %0, %10, %12, vcc" AGX_DPP_TAKE "v_cndmask_b32_dpp %1, %11, %12, vcc" AGX_DPP_TAKE                \
        "v_cndmask_b32_dpp %2, %2, %4, vcc" AGX_DPP_TAKE "v_cndmask_b32_dpp %3, %3, %5, vcc" AGX_DPP_TAKE                    \
        : "=&v"(zl), "=&v"(fl), "+v"(ta), "+v"(tb), "=&v"(ma), "=&v"(mb)                                                     \
        : "v"(rowsA), "v"(rowsB), "v"(kv), "s"(start_mask), "v"(z_last), "v"(f_last), "v"(z0v)                               \
        : "vcc")

template <int K>
__device__ __forceinline__ void fast_head(uint32_t &zl, uint32_t &fl, uint32_t &ta, uint32_t &tb, uint32_t rowsA, uint32_t rowsB,
                                          uint32_t kv, uint64_t start_mask, uint32_t z_last, uint32_t f_last, uint32_t z0v)
{
    uint32_t ma, mb;
    if constexpr (K == 1)
        AGX_FAST_HEAD("BYTE_1");
    else if constexpr (K == 2)
        AGX_FAST_HEAD("BYTE_2");
    else if constexpr (K == 3)
        AGX_FAST_HEAD("BYTE_3");
    else
        AGX_FAST_HEAD("BYTE_0");
}

// general: the image holds the symbols themselves (zero beyond a sequence -- byte 0 is no symbol, and padding
// COLUMNS carry 0x100 << shift, which is no byte either); byte k of the two quads -> {a, 0, b, 0} << shift
__device__ __forceinline__ void bytes_head(uint32_t &zl, uint32_t &fl, uint32_t &yc, uint32_t rowsA, uint32_t rowsB, uint32_t sel,
                                           uint32_t sh_sym, uint64_t start_mask, uint32_t z_last, uint32_t f_last, uint32_t z0v)
{
    uint32_t fresh;
    asm("v_perm_b32 %3, %5, %4, %6\n"
        "v_lshlrev_b32 %3, %7, %3\n"
        "s_mov_b64 vcc, %8\n"
        "v_cndmask_b32_dpp %0, %9, %11, vcc" AGX_DPP_TAKE "v_cndmask_b32_dpp %1, %10, %11, vcc" AGX_DPP_TAKE
        "v_cndmask_b32_dpp %2, %2, %3, vcc" AGX_DPP_TAKE
        : "=&v"(zl), "=&v"(fl), "+v"(yc), "=&v"(fresh)
        : "v"(rowsA), "v"(rowsB), "s"(sel), "v"(sh_sym), "s"(start_mask), "v"(z_last), "v"(f_last), "v"(z0v)
        : "vcc");
}

// FAST = the wave's pairs all passed the pack kernel's DNA test (agx_sw_pack_kernel.hip, sw_pack_dna): at most four
// distinct symbols in the shorter sequence, a trailing newline sentinel at most at the very end of either.  The
// image then holds CODES, the sentinels stripped:
//   x  as v_perm_b32 selector bytes -- code 0..3 for pair A, 4 + code for pair B, 0x0c (the constant 0) for a padding
//      column -- RIGHT-aligned in the group's G * C columns: padding columns on the left behave exactly like column
//      0 (H = 0, Q = -inf), and the last symbol always sits in the last column of the group's last lane;
//   y  as shift counts (fast_head).
// The row table M (byte c = delta if the row symbol is x's code c, else 0) travels down the lanes, and ONE
// v_perm_b32 per column yields the match bonus of BOTH pairs (selector byte 0 picks M_A[code], byte 2 picks
// M_B[code]) where the general cell spends v_xor_b32 + v_pk_min_u16: 9.5 instead of 10.5 instructions per two
// cells.  The stripped sentinels are put back at the end: a final newline aligns with nothing but the other
// sequence's final newline, so the score is max(best, H[lx'][ly'] + match) when both had one
// (antidiagonalSmithWaterman.c:229-247 keeps the newline as a symbol; SURVEY.md Q1), best otherwise.  H[lx'][ly']
// is what the group's last lane holds in its last column after step ly' - 1 + (G - 1).
//
// RISE = "rising offsets": every stored value additionally carries an offset that grows by |ge| per step, the same in
// all lanes: r(t) = (t + 2) |ge|, on z of step t; r(t - 1) on e, f and H of step t.  The vertical gap then needs no
// subtraction at all -- P_new + r(t) = max(z_up + r(t), (P + r(t-1))) since r(t) - |ge| = r(t - 1) -- the horizontal gap
// subtracts after its maximum instead of before, the diagonal is unchanged (z_diag carries r(t - 1), which is H's
// offset), and z = H - (|gf| - |ge|).  One v_sub_u32 less per two cells; per STEP the floor, the column-0 value
// (wave-uniform: a scalar add) and the running maximum rise by |ge|.  What a lane takes over from its left
// neighbour was made one step earlier and is |ge| behind: in the lane's first column that lag cancels the horizontal
// gap's subtraction (max(z_left + |ge|, f_left + |ge|) - |ge|), and the diagonal adds |ge| through its constant.
// The host asks for this variant when B + the largest score + (steps + 2) |ge| stays
// below 0x7c00 (agx_sw.cpp) -- rows up to about 27 000 with the reference's scores; beyond, the plain cell.
//
// KC = column classes of the rising cell (0: plain cell, 1: rising, 4: rising with classes).  With KC = 4 column j of a
// lane additionally carries (j mod 4) |ge|: from one column to the next the offset rises by |ge|, which is exactly what
// the horizontal gap subtracts -- f = max(z_left, f) with no subtraction, except where the class wraps (every fourth
// column: minus 4 |ge|) -- and the diagonal adds |ge| through its constant (minus 3 |ge| at a wrap: the host asks for
// this variant only when mismatch + |gf| >= 3 |ge|, so that constant is not negative).  The floor exists once per class
// and rises by |ge| per step.  What a lane hands to its right neighbour still carries the last column's class offset
// c_end: the lane's first column takes it off once, after the horizontal gap's maximum (max(z - c, f - c) =
// max(z, f) - c), and its diagonal through its constant (hdf = hd0 - c_end).  Per column (two cells) 6 + 1/4 + 1/2
// instructions, against 7 + 1/2.
//
// WIDE: the class period P is C / 2 instead of four (column j carries (j mod P) |ge|; "KC = 4" stays the name of "rising with
// column classes").  A lane then wraps once a step, every class holds exactly two columns, and the wrap's and the first
// column's diagonal constants are negative: hdw = mismatch + |gf| + |ge| - P |ge|, hdf = hd0 - (P - 1) |ge|.  They go in as
// the two's complement of k * 0x10001 in the 32-bit add the cell issues anyway, which is exact in both halves because both
// RESULTS lie in [0, 0x10000) -- they are stored values of class 0 (DESIGN.md 4.1 has the argument and the host's rule).
// Everything below is written in terms of NK = P.
//
// The running maximum of KC = 4 is kept per OFFSET rather than per class: z of step t in class k carries
// (t + 2 + k) |ge|, so inside a quad of steps (t = t0 + s) every z of class k at phase s shares the offset of
// maximum m = s + k, m = 0 .. KC + 2.  The KC + 3 maxima rise by 4 |ge| once per quad (7 instructions a quad where four
// classes rising every step took 16), and they take each step's z one step LATE, from the values the next step's cells
// read anyway: the chain of maxima then has the whole step to run in, not the few instructions left behind the last
// column, where each dependent v_pk_maximum3_f16 drew an s_nop.  The tail steps (steps mod 4) run at phase 0 and
// rotate the maxima by one place after each step; the last step's z are taken behind the loop.
//
// ST = wave stamps, for tools/sw_wave_timeline.hip alone: a diagnostic build hands in an object whose take<K>() reads the cycle
// counter at place K of the wave -- 1 in front of the first quad of steps, 2 behind the last step, 3 in front of the result
// store (0 and what follows the store are the diagnostic kernel's own).  The library's kernels pass none: SwNoStamps::take is
// empty, and their code is instruction for instruction what it is without the parameter.
struct SwNoStamps {
    template <int K>
    __device__ __forceinline__ void take() const {}
};

template <int C, bool FAST, int KC, bool WIDE = false, bool STAGED = false, class ST = SwNoStamps>
__device__ __forceinline__ void pk2_fill(const SwParams &prm, const uint32_t *__restrict__ img, const SwGroup2 &g, const SwWave &w,
                                         int32_t *__restrict__ scores, int lane, int G, int gl, bool active, bool start, bool feeder,
                                         const ST &st = ST{})
{
    constexpr int XW = (C + 3) / 4; // dwords holding this lane's C symbols
    constexpr bool RISE = KC > 0;
    constexpr int NK = KC > 1 ? (WIDE ? C / 2 : KC) : 1; // the class period: floors kept (WIDE: see sw_pk2_period, agx_sw.h)
    constexpr int kEnd = KC > 1 ? (C - 1) % NK : 0;   // class of the lane's last column
    constexpr int NM = KC > 1 ? NK + 3 : NK;          // running maxima kept: KC > 1, one per offset within a quad of steps
    const uint32_t sh_sym = prm.shift;         // general: symbols live as byte << shift
    const uint32_t col_pad = 0x100u << sh_sym; // never equals (byte << shift)
    const uint32_t ge = in_vgpr(prm.age2), gf = in_vgpr(RISE ? prm.agf2 - prm.age2 : prm.agf2); // |ge|; |gf| (RISE: |gf| - |ge|)
    const uint32_t hd = in_vgpr(FAST ? prm.hd2 - prm.delta2 : prm.hd2);                // mismatch + |gf| / match + |gf|
    const uint32_t bias = prm.bias2, delta = prm.delta2;
    const uint32_t z0 = prm.bias2 - prm.agf2; // H = 0 as the state both gap recurrences read (z = H + gf), both halves
    const uint32_t hd0 = in_vgpr((FAST ? prm.hd2 - prm.delta2 : prm.hd2) + (RISE ? prm.age2 : 0u)); // first column's diagonal; KC > 1: every non-wrapping one's
    const uint32_t hdw = in_vgpr((FAST ? prm.hd2 - prm.delta2 : prm.hd2) + prm.age2 - (uint32_t)NK * prm.age2); // KC > 1: a wrapping column's diagonal
    const uint32_t ge_wrap = in_vgpr((uint32_t)NK * prm.age2), c_end = in_vgpr((uint32_t)kEnd * prm.age2);
    // KC > 1: the first column's diagonal, which takes off the class offset its left neighbour's last column carried
    // (hd0 - c_end >= mismatch + |gf| - 2 |ge| >= 0 in both halves at the period of four; WIDE: negative, see above)
    const uint32_t hdf = KC > 1 && kEnd > 0 ? in_vgpr((FAST ? prm.hd2 - prm.delta2 : prm.hd2) + prm.age2 - (uint32_t)kEnd * prm.age2) : hd0;
    const uint32_t ge4 = in_vgpr(4u * prm.age2); // KC > 1: what the maxima rise by per quad of steps
    uint32_t zb = (RISE ? z0 + prm.age2 : z0) + (uint32_t)kEnd * prm.age2; // column 0 as the first lane takes it over: z0 + r(t - 1) (+ what every lane takes off on arrival)
    // WIDE: the floors are kept per OFFSET within a quad of steps, like the maxima -- class k at phase s reads floor s + k --
    // and rise by 4 |ge| once a quad: NM scalar adds a quad where a floor per class rising every step took 4 NK (22 for 76
    // at 38 columns; at the period of four, 7 for 12, there was nothing to save)
    constexpr bool FQ = WIDE && KC > 1;
    constexpr int NF = FQ ? NM : NK;
    uint32_t floorv[NF];                                          // P~ >= 0 at H's offset: B + r(t - 1) (+ class); in VGPRs: as an
#pragma unroll                                                    // SGPR operand it drew an s_nop after every group of four
    for (int k = 0; k < NF; ++k) floorv[k] = (RISE ? bias + prm.age2 : bias) + (uint32_t)k * prm.age2;
    const uint32_t z_init = RISE ? z0 + prm.age2 : z0;            // H = 0 one step before the first: z0 + r(-1)
    const uint32_t kv = in_vgpr((prm.delta2 & 0xffu) << 24); // FAST: the table source
    const uint64_t start_mask = __ballot(start);
    const uint32_t lx_mask = FAST ? 0xfffu : 0x7fffu;
    const int lxA = (int)(g.lx_ly[0] & lx_mask), lxB = (int)(g.lx_ly[1] & lx_mask);
    const int lyA = (int)(g.lx_ly[0] >> 16), lyB = (int)(g.lx_ly[1] >> 16);

    // The row stream: quad q (rows 4q .. 4q + 3) of pair A / pair B.  Every lane loads, unconditionally, quad
    // min(q, last) of its half -- word 0 of the zero block when the half has no rows (vacant, idle lane, empty y) --
    // so that the load is one instruction of the straight-line step code, not a branch of its own.  Only the group's
    // first lane uses what it read, and only while q < nq (row_sel); everything else reads as "matches nothing".
    // row_sel is applied where the quad is used, a quad of steps after the load: applied next to the load, it would
    // draw the wait for the load there.
    const uint32_t no_row = FAST ? 0x1f1f1f1fu : 0u; // rows beyond the sequence match nothing
    const uint32_t *ybA = lyA > 0 ? img + g.y_dw[0] : img, *ybB = lyB > 0 ? img + g.y_dw[1] : img;
    const uint32_t lastA = lyA > 0 ? (uint32_t)((lyA + 3) >> 2) - 1u : 0u, lastB = lyB > 0 ? (uint32_t)((lyB + 3) >> 2) - 1u : 0u;
    const int nqA = feeder ? (lyA + 3) >> 2 : 0, nqB = feeder ? (lyB + 3) >> 2 : 0;
    auto loadA = [&](int q) -> uint32_t { return ybA[min((uint32_t)q, lastA)]; };
    auto loadB = [&](int q) -> uint32_t { return ybB[min((uint32_t)q, lastB)]; };
    auto row_selA = [&](int q, uint32_t v) -> uint32_t { return q < nqA ? v : no_row; };
    auto row_selB = [&](int q, uint32_t v) -> uint32_t { return q < nqB ? v : no_row; };

    // this lane's C symbols of both short sequences -> one register per column:
    //   general: (a << shift) | (b << shift) << 16;   FAST: the v_perm_b32 selector {sel_a, 0x0c, sel_b, 0x0c}
    uint32_t xq[C];
    // quads in flight: narrow lanes run a quad of steps in fewer than 200 instructions (C = 4: about 175) and keep two
    constexpr int PF = C < 8 ? 2 : 1;
    uint32_t nextA[PF], nextB[PF]; // the quads the next PF quads of steps read, as loaded (before row_sel)
    {
        const uint32_t o = (uint32_t)gl * C, d0 = o >> 2, sh = o & 3u;
        // FAST: a vacant half and idle lanes (their records point at the zero block, offset 0: pk2_body zeroes idle lanes'
        // records) read zeros there -- at most word (G C + 3) / 4 of the kSwPackedMaxShort / 4 + 1 -- and become
        // all padding.  Every word of both halves and the first row quads go out back to back, then ONE wait.
        const uint32_t fillA = (FAST && !(active && g.x_dw[0])) ? 0x0c0c0c0cu : 0u;
        const uint32_t fillB = (FAST && !(active && g.x_dw[1])) ? 0x0c0c0c0cu : 0u;
        uint32_t ra[XW + 1], rb[XW + 1];
#pragma unroll
        for (int k = 0; k <= XW; ++k) {
            ra[k] = img[g.x_dw[0] + d0 + k];
            rb[k] = img[g.x_dw[1] + d0 + k];
        }
#pragma unroll
        for (int r = 0; r < PF; ++r) {
            nextA[r] = loadA(r);
            nextB[r] = loadB(r);
        }
        __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k <= XW; ++k) {
            ra[k] |= fillA;
            rb[k] |= fillB;
        }
#pragma unroll
        for (int k = 0; k < XW; ++k) {
            const uint32_t a = __builtin_amdgcn_alignbyte(ra[k + 1], ra[k], sh);
            const uint32_t b = __builtin_amdgcn_alignbyte(rb[k + 1], rb[k], sh);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * k + i < C) {
                    const uint32_t ca = (a >> (8 * i)) & 0xffu, cb = (b >> (8 * i)) & 0xffu;
                    uint32_t v;
                    if constexpr (FAST)
                        v = ca | 0x0c00u | (cb << 16) | 0x0c000000u;
                    else {
                        const int col = (int)o + 4 * k + i;
                        v = (col < lxA ? ca << sh_sym : col_pad) | ((col < lxB ? cb << sh_sym : col_pad) << 16);
                    }
                    // opaque to the compiler: left visible, it keeps the length tests as lane masks and rebuilds
                    // every register in every step to save registers
                    asm volatile("" : "+v"(v));
                    xq[4 * k + i] = v;
                }
        }
    }

    // state per owned column, both pairs packed, biased: z = H + gf + B and e = max(P, 0) + B
    uint32_t z[C], e[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        z[j] = z_init + (uint32_t)(j % NK) * prm.age2;
        e[j] = bias + (uint32_t)(j % NK) * prm.age2; // anything up to the first floor
    }
    // the horizontal gap state needs no clamp: Q >= z_left >= gf always; "no gap open yet" is Q = gf,
    // whose successor gf + ge loses against every z_left
    uint32_t z_last = z_init + (uint32_t)kEnd * prm.age2, f_last = z_last, diag_in = z0 + (uint32_t)kEnd * prm.age2;
    // :335.  KC > 1: one per offset, maximum m at (t0 + 2 + m) |ge| in the quad of steps t0 .. t0 + 3 (H = 0 to begin
    // with); otherwise one per class, at z's offset of the step
    uint32_t best[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) best[k] = z_init + (uint32_t)(KC > 1 ? k + 1 : k) * prm.age2;
    uint32_t yc = 0;         // general: the row symbols of both pairs
    uint32_t ta = 0, tb = 0; // FAST: the row tables of pair A / pair B

    // FAST: the step after which the group's last lane holds H[lx'][ly'] in its last column (bit 13 of the record:
    // both sequences ended with the sentinel); a stripped side that is empty leaves the corner at H = 0
    const bool last = active && gl == G - 1;
    const bool nlA = FAST && last && ((g.lx_ly[0] >> 13) & 1u), nlB = FAST && last && ((g.lx_ly[1] >> 13) & 1u);
    const int capA_t = (nlA && lxA > 0 && lyA > 0) ? lyA + G - 2 : -1, capB_t = (nlB && lxB > 0 && lyB > 0) ? lyB + G - 2 : -1;
    uint32_t cornerA = z_init + (uint32_t)kEnd * prm.age2, cornerB = cornerA; // (taken from the last column: its class offset comes off at the end)

    const int steps = (int)w.steps;
    uint32_t rowsA = 0, rowsB = 0;
    int t = 0;

    // KC > 1: z of phase S go to the maxima S .. S + KC - 1, every class's columns two at a time
    auto take_max = [&](auto sc) __attribute__((always_inline)) {
        constexpr int S = decltype(sc)::value;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int j = k; j < C; j += 2 * NK) {
                if (j + NK < C)
                    best[S + k] = umax3(best[S + k], z[j], z[j + NK]);
                else
                    best[S + k] = umax2(best[S + k], z[j]);
            }
        }
    };

    // K = which byte of the quads this step reads (the tail loop shifts the quads instead: K = 0); S = the step's phase
    // in its quad for the maxima of KC > 1 (S = 4: a tail step, which rotates the maxima instead); CAP = look for the corner.
    // KC > 1: phases 1 .. 3 take the previous step's z before their cells overwrite them; phase 3 and the tail take
    // their own z behind their cells as well.
    auto step = [&](auto kc, auto sc, auto cc) __attribute__((always_inline)) {
        constexpr int K = decltype(kc)::value;
        constexpr int S = decltype(sc)::value;
        constexpr bool CAP = decltype(cc)::value;
        uint32_t zl, fl;
        if constexpr (FAST)
            fast_head<K>(zl, fl, ta, tb, rowsA, rowsB, kv, start_mask, z_last, f_last, zb);
        else
            bytes_head(zl, fl, yc, rowsA, rowsB, 0x0c040c00u + 0x00010001u * K, sh_sym, start_mask, z_last, f_last, zb);
        if constexpr (KC > 1 && S > 0 && S < 4)
            take_max(std::integral_constant<int, S - 1>{});
        else if constexpr (KC <= 1 && RISE)
            best[0] += ge;
        uint32_t zd = diag_in; // H[r-1][first column - 1] + gf
        diag_in = zl;
        uint32_t zleft = zl, f = fl;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const bool wrap = KC > 1 && j > 0 && j % NK == 0; // compile-time after unrolling
            const uint32_t up = z[j];
            uint32_t ev; // reference P, :313, clamped at 0;  reference Q, :321
            if constexpr (RISE) {
                ev = umax3(up, e[j], floorv[(FQ && S < 4 ? S : 0) + j % NK]);
                f = umax2(zleft, f);
                if (KC == 1 && j > 0) f -= ge; // (first column: see above)
                if (KC > 1 && kEnd > 0 && j == 0) f -= c_end;
                if (wrap) f -= ge_wrap;
            } else {
                ev = umax3(up, e[j] - ge, bias);
                f = umax2(zleft, f - ge);
            }
            const uint32_t hdc = KC > 1 ? (wrap ? hdw : j ? hd0 : hdf) : (j ? hd : hd0);
            uint32_t u;                                        // H_diag + match / + mismatch, :332
            if constexpr (FAST)
                u = (zd + hdc) + __builtin_amdgcn_perm(tb, ta, xq[j]); // mismatch, plus delta on a match
            else
                u = (zd + hdc) - umin2(xq[j] ^ yc, delta); // match, minus delta on a mismatch
            const uint32_t v = umax3(ev, f, u);                // :333 (ev >= B carries the zero floor)
            const uint32_t zn = v - gf;
            e[j] = ev;
            z[j] = zn;
            zd = up;
            zleft = zn;
        }
        // :335
        if constexpr (KC <= 1) {
#pragma unroll
            for (int j = 0; j < C; j += 2) best[0] = umax3(best[0], z[j], z[j + 1]);
        } else if constexpr (S >= 3)
            take_max(std::integral_constant<int, S == 3 ? 3 : 0>{});
        if constexpr (FAST && CAP) {
            cornerA = t == capA_t ? zleft : cornerA;
            cornerB = t == capB_t ? zleft : cornerB;
        }
        z_last = zleft;
        f_last = f;
        if constexpr (RISE) {
            if constexpr (!FQ || S == 4) { // (FQ: a tail step moves every offset one step on)
#pragma unroll
                for (int k = 0; k < NF; ++k) floorv[k] += prm.age2;
            }
            zb += prm.age2;
        }
        ++t;
    };

    // The row stream runs PF quads ahead: the load issued at the top of a quad is first read at the top of the quad PF
    // later -- four steps, about 1100 instructions at C = 38 -- so the wait the compiler places there finds it landed.
    // rowsA / rowsB are made before the load: the steps' heads read registers that no load is pending on.  With
    // PF = 2 the loop takes two quads with a register each (copying one into the other would draw the wait one
    // quad early).
    auto rise4 = [&]() __attribute__((always_inline)) {
        if constexpr (KC > 1) {
#pragma unroll
            for (int m = 0; m < NM; ++m) best[m] += ge4;
        }
        if constexpr (FQ) {
#pragma unroll
            for (int m = 0; m < NF; ++m) floorv[m] += 4u * prm.age2;
        }
    };
    // (the rise at the quad's end: at its start the scheduler left the last step's cells more s_nop)
    auto quad_of_steps = [&](auto cc) __attribute__((always_inline)) {
        step(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, cc);
        step(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, cc);
        step(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}, cc);
        step(std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{}, cc);
        rise4();
    };
    // Staged priority (STAGED; DESIGN.md 4.1, profiles/sw_wave_timeline.md).  Of the two waves of a SIMD the older one takes
    // nearly every issue slot: left alone it leaves its loop when the younger has done a tenth of its own, and the younger then
    // runs the rest alone.  With the staging a wave lowers its own priority as it advances -- s_setprio 3, 2, 1, 0 at the
    // boundaries of four segments of its quads -- so the wave that lags has the higher priority and the pair stays together to
    // within a segment.  The segments shrink (boundaries at 1/2, 3/4, 7/8 of the quads; prm.stage == 2, the tool's comparison:
    // equal quarters), which bounds what the last wave runs alone.  One uniform scalar compare and branch a quad, nothing per
    // step; the host asks for it only for a launch whose waves are all resident at once (agx_sw.cpp): where new waves back-fill,
    // a wave near its end must not lose to a fresh one.  It is a build of its own, in kernels of its own (sw_fill_pk2w_staged,
    // ...): in the mixed batches' launches, which are not staged, even that compare cost 0.2 %.
    const int quads = steps >> 2;
    int stage_at = 0, stage_lv = 3;
    auto staging = [&](int q) __attribute__((always_inline)) {
        if (STAGED && q == stage_at) {
            const bool even = prm.stage == 2;
            int next = -1;
            switch (stage_lv) {
            case 3: __builtin_amdgcn_s_setprio(3); next = even ? quads >> 2 : quads >> 1; break;
            case 2: __builtin_amdgcn_s_setprio(2); next = even ? quads >> 1 : (3 * quads) >> 2; break;
            case 1: __builtin_amdgcn_s_setprio(1); next = even ? (3 * quads) >> 2 : (7 * quads) >> 3; break;
            default: __builtin_amdgcn_s_setprio(0); break;
            }
            stage_at = stage_lv > 0 ? max(next, q + 1) : -1;
            --stage_lv;
        }
    };
    auto take = [&](int q, int r) __attribute__((always_inline)) {
        staging(q);
        rowsA = row_selA(q, nextA[r]);
        rowsB = row_selB(q, nextB[r]);
        nextA[r] = loadA(q + PF);
        nextB[r] = loadB(q + PF);
        // WIDE: the loads stay here.  With 22 maxima live the scheduler otherwise sinks them towards the quad's end to save two
        // registers (the one-launch kernel at 34 and 36 columns: 165 instructions ahead of their wait)
        if constexpr (WIDE) __builtin_amdgcn_sched_barrier(0);
    };
    // FAST: the corner falls at step capA_t / capB_t of a group's last lane, so the quads before the wave's first such
    // step run without looking for it (a loop of their own: a branch around the test inside the loop is if-converted)
    int cap_first = 0x7fffffff;
    if constexpr (FAST) {
        cap_first = min(capA_t < 0 ? 0x7fffffff : capA_t, capB_t < 0 ? 0x7fffffff : capB_t);
        for (int o = 32; o > 0; o >>= 1) cap_first = min(cap_first, __shfl_xor(cap_first, o));
        cap_first = __builtin_amdgcn_readfirstlane(cap_first);
    }
    const int quads_free = min(quads, cap_first >> 2);
    constexpr std::integral_constant<bool, false> no_cap{};
    constexpr std::integral_constant<bool, FAST> cap{};
    st.template take<1>();
    int q = 0;
    if constexpr (PF == 1) {
        if constexpr (FAST) {
            for (; q < quads_free; ++q) {
                take(q, 0);
                quad_of_steps(no_cap);
            }
        }
        for (; q < quads; ++q) {
            take(q, 0);
            quad_of_steps(cap);
        }
    } else {
        if constexpr (FAST) {
            for (; q + 1 < quads_free; q += 2) {
                take(q, 0);
                quad_of_steps(no_cap);
                take(q + 1, 1);
                quad_of_steps(no_cap);
            }
        }
        for (; q + 1 < quads; q += 2) {
            take(q, 0);
            quad_of_steps(cap);
            take(q + 1, 1);
            quad_of_steps(cap);
        }
        if (q < quads) { // an odd number of quads
            rowsA = row_selA(q, nextA[0]);
            rowsB = row_selB(q, nextB[0]);
            quad_of_steps(cap);
            ++q;
            nextA[0] = nextA[1];
            nextB[0] = nextB[1];
        }
    }
    rowsA = row_selA(q, nextA[0]);
    rowsB = row_selB(q, nextB[0]);
#pragma unroll 1
    while (t < steps) {
        step(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{}, cap);
        rowsA >>= 8;
        rowsB >>= 8;
        if constexpr (KC > 1) { // one step on: maximum m + 1 becomes maximum m, maximum 0 moves to the top
            const uint32_t b0 = best[0];
#pragma unroll
            for (int m = 0; m + 1 < NM; ++m) best[m] = best[m + 1];
            best[NM - 1] = b0 + (uint32_t)NM * prm.age2;
        }
    }
    st.template take<2>();
    if constexpr (KC > 1) { // the maxima now stand at (steps + 2 + m) |ge|: all to the top one's offset, then to r(steps - 1)
#pragma unroll
        for (int m = 0; m + 1 < NM; ++m) best[NM - 1] = umax2(best[NM - 1], best[m] + (uint32_t)(NM - 1 - m) * prm.age2);
        best[0] = best[NM - 1] - (uint32_t)NM * prm.age2;
    }

    if constexpr (FAST) {
        // the stripped sentinels: when both sequences ended with one, the two newlines align after the corner cell.
        // H_corner + match as a z value is z_corner + match.
        const uint32_t match2 = prm.hd2 - prm.agf2; // (match + |gf|) - |gf| in both halves
        const uint32_t ge1 = RISE ? prm.age2 & 0xffffu : 0u; // the corner was taken at offset r(cap_t), best stands at r(steps - 1)
        const uint32_t off_end = (uint32_t)kEnd * (prm.age2 & 0xffffu);
        uint32_t cand = best[0];
        if (nlA) cand = (cand & 0xffff0000u) | ((cornerA + match2 + (uint32_t)(steps - 1 - capA_t) * ge1 - off_end) & 0xffffu);
        if (nlB) cand = (cand & 0xffffu) | ((cornerB + match2 + (((uint32_t)(steps - 1 - capB_t) * ge1 - off_end) << 16)) & 0xffff0000u);
        best[0] = umax2(best[0], cand);
    }
    uint32_t bestv = best[0];
    // max over the group's lanes (G need not be a power of two), both halves at once
    for (int o = 1; o < G; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_down((int)bestv, o);
        if (gl + o < G) bestv = umax2(bestv, other);
    }
    {
        const int off = (int)(z0 & 0xffffu) + (RISE ? (steps + 1) * (int)(prm.age2 & 0xffffu) : 0); // stored value of H = 0, at r(steps - 1)
        // The wave's results move to its first lanes -- lane i takes group i's two scores from that group's first lane --
        // and go out from there: neighbouring pairs as ONE 8-byte store per group, so that in a batch planned in file order
        // adjacent lanes write adjacent bytes and the wave's scores leave as one request (one PCIe write when the scores
        // array is the caller's page-locked one, agx_sw_batch_bind_scores; the spare slot n_pairs a vacant half points at
        // does not exist there).
        const int src = (lane * G) & 63;
        const int sa = __shfl((int)(bestv & 0xffffu) - off, src), sb = __shfl((int)(bestv >> 16) - off, src);
        const uint32_t oa = (uint32_t)__shfl((int)g.out[0], src), ob = (uint32_t)__shfl((int)g.out[1], src);
        st.template take<3>();
        if (lane < (int)w.n_groups) {
            if (ob == oa + 1u && !(oa & 1u) && ob < prm.n_out)
                *reinterpret_cast<int2 *>(scores + oa) = make_int2(sa, sb);
            else {
                scores[oa] = sa;
                if (ob < prm.n_out) scores[ob] = sb;
            }
        }
    }
}

template <int C, int KC, bool WIDE = false, bool STAGED = false, class ST = SwNoStamps>
__device__ __forceinline__ void pk2_body(const SwParams &prm, const uint32_t *__restrict__ img, const SwGroup2 *__restrict__ groups,
                                         const SwWave w, int32_t *__restrict__ scores, const ST &st = ST{})
{
    static_assert(C % 2 == 0, "the running maximum takes two columns per instruction");
    // column classes cost ten instructions a step and save three quarters of one per column: narrow lanes do without
    constexpr int KCC = KC > 1 && C < 14 ? 1 : KC;
    constexpr bool W = WIDE && KCC > 1 && sw_pk2_period(C) > 4; // (classes whose wide build does not fit keep the period of four)
    const int lane = threadIdx.x & 63;
    const int G = w.G;
    const int grp = lane / G;
    const int gl = lane - grp * G;
    const bool active = grp < (int)w.n_groups;
    const bool start = gl == 0;
    const bool feeder = active && start;

    // idle lanes read the wave's first record (no branch around the load, one wait) and zero it: their image reads
    // then go to the zero block
    SwGroup2 g = groups[w.first_group + (active ? grp : 0)];
    __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        g.x_dw[k] = active ? g.x_dw[k] : 0u;
        g.y_dw[k] = active ? g.y_dw[k] : 0u;
        g.lx_ly[k] = active ? g.lx_ly[k] : 0u;
        g.out[k] = active ? g.out[k] : 0u;
    }
    // bit 16 of the wave record's class word: set by the pack kernel when every pair of the wave is DNA-coded
    if (__builtin_amdgcn_readfirstlane(w.reserved >> 16) & 1u)
        pk2_fill<C, true, KCC, W, STAGED>(prm, img, g, w, scores, lane, G, gl, active, start, feeder, st);
    else
        pk2_fill<C, false, KCC, W, STAGED>(prm, img, g, w, scores, lane, G, gl, active, start, feeder, st);
}

} // namespace
