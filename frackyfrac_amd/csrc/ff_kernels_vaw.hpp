// ff_kernels_vaw.hpp -- variance-adjusted weighted UniFrac, "VAW" (Chang, Luan & Sun 2011): binary32 terms, binary64 sums.
// A fragment of ff_dev_run.hip: included there, once, inside its anonymous namespace, behind ff_kernels_general.hpp
// (whose XW_* / G_F32 helpers it uses).
//
// The flat nodes carry UNDIVIDED subtree sums x_s(b).  Per sample T_s = its largest abundance (the root's sum),
// p_s(b) = x_s(b) / T_s, c_s(b) = T_s - x_s(b) (T_s where the sample has not the branch); per pair and branch
//     m = x_i + x_j,  r = c_i + c_j,  and over the branches with m r > 0 only
//     numer = sum_b l |p_i - p_j| / sqrt(m r)      denom = sum_b l (p_i + p_j) / sqrt(m r)      d_VAW = numer / denom.
// This is the paper's normalisation (p = x / T, true proportions), deliberately NOT a re-weighting of the divisor of
// the reference's normalizeFlatNodes.  The weight 1 / sqrt(m r) depends on BOTH samples: not an L1 distance, not a
// contraction, and pair_general_kernel's trick -- a one-sided term is a constant of the column -- does not carry over
// either, because even a one-sided term has the OTHER sample's total under the root: l p_j / sqrt(x_j (T_i + c_j)).
// What does carry over is the split of that term: q_j = l p_j / sqrt(x_j) belongs to the column alone and is staged
// (binary64, rounded once); the kernel supplies rsq(T_i + c_j).
//
// Staged (stage_vaw_kernel, ff_kernels_stage.hpp), branch-major, one cell per (row, sample), in TWO planes of 8 bytes:
//     plane A  (x, c)   x = 0 and c = T_s where the sample has not the branch (EVERY cell of a column carries c);
//                       c exactly 0 where x == T_s
//     plane B  (p, q)   both 0 where the sample has not the branch
// and per sample (T, 1 / T).  A wave owns an H x 64 pair tile, a lane one column.  Per branch the lane loads its own
// cell of both planes (two 8-byte vector loads) and the wave the H row cells of plane A ONLY (scalar loads, 8 H bytes:
// the scalar-cache traffic of pair_general_kernel, not twice that): the row's p is x_i (1 / T_i), one multiplication,
// and the staging forms the column's p by THE SAME binary32 multiplication of the same operands, so that the p of
// twins are equal bit for bit (d = 0 exactly).  Why two planes and not 16-byte cells: the kernel holds two operand
// sets (one branch ahead); 16-byte row cells are 2 x 16 x 4 = 128 scalar registers at H = 16, and the file has 102.
// That settled it before any run; the one-plane layout was never built.  For the same reason T_i and 1 / T_i, uniform
// values loaded once per tile through scalar loads, are KEPT in vector registers (2 H of them).
//
// Per branch, by the row's x -- a scalar --:
//     row has not the branch (chain X):  r = T_i + c_j,  t = q_j rsq(r), t = 0 where r == 0,  numer += t,  denom += t
//         (one add, one v_rsq_f32, one multiply, compare + select, one convert, two v_add_f64.  A lane whose own y is 0
//          has q = 0 and adds +0; r == 0: the row's sample is empty and the column's sits wholly under this branch)
//     row has it (chain Y):  m = x_i + y_j,  r = c_i + c_j,  w = l rsq(m r), w = 0 where r == 0 (the branch holds
//         everything of both samples),  p_i = x_i (1 / T_i),  numer += |p_i - p_j| w,  denom += (p_i + p_j) w
//         (a lane without the branch has p_j = 0: d == s bit for bit, the two addends are equal -- an empty sample
//          against any other gives a quotient of exactly 1)
//
// Range.  v_rsq_f32 takes no denormals and m r must neither overflow nor underflow.  The staging multiplies all
// abundances by ONE power of two that puts the largest T into [2^31, 2^32) -- d_VAW is invariant under it, both sums
// scale by the same factor -- and raises every non-zero x, c and T below 2^-60 to 2^-60 (a non-zero q below the
// smallest normal number to that number): 2^-120 <= m r <= 2^67, and p >= 2^-93.  A table whose abundances span more
// than 2^91 (2.5e27) below its largest total has its smallest values replaced in that way: presence is kept, the
// bound below is not claimed for the terms they are in.  Branch lengths are used as binary32 numbers, as in
// pair_general_kernel: one beyond that range makes the distances it takes part in NaN.
//
// Accuracy.  Every term is non-negative, so the relative error of either sum is at most the largest
// relative error of a term; the sums are binary64.  Unit u = 2^-24 (one rounding); v_rsq_f32 is good to one ulp = 2 u.
//     chain Y, denominator term l (p_i + p_j) rsq(m r):
//         p: x 1, 1 / T 1, product 1 = 3 (both p alike); s = p_i + p_j: 3 + 1 = 4
//         m: inputs 1, add 1 = 2; r likewise 2; m r: 2 + 2 + 1 = 5; the root halves it, 2.5, the instruction adds 2: 4.5
//         l as binary32 1; l rsq 1; times s 1: 3                                              total 11.5
//       numerator term: the only cancellation, d = |p_i - p_j|, is off by at most 3 u p_i + 3 u p_j + u d <= 4 u s,
//       i.e. 4 u of the MATCHING denominator term, where s had 4: the same 11.5.
//     chain X, t = q rsq(T_i + c_j): q 1; r: 1 + 1 = 2, halved 1, instruction 2: 3; product 1  total 5
// With d_VAW <= 1 the result is within (roundings per term + 2) u <= 14 * 2^-24 = 8.4e-7 absolute: under the 1e-6 of
// FF_PRECISION_FLOAT32.
//
// Control flow, hazards and order of summation are pair_general_kernel's: the H rows of a branch are one asm block of
// the two chains (XW_CHAIN / XW_ROWS of ff_kernels_exact_w.hpp), a branch instruction is taken only where consecutive
// rows differ; every v_rsq_f32 is followed by its s_nop; binary64 accumulators (4 H registers); every wave walks ALL
// staged rows in ascending order, so a pair's bits do not depend on tile height, shard or launch.

// chain X: t0 = r, t1 = t
#define VW_ONE(R) "v_add_f32 %[t0], %[T" #R "], %[cj]\n" "v_rsq_f32 %[t1], %[t0]\n" "s_nop 0\n" "v_cmp_lt_f32 vcc, 0, %[t0]\n" \
                  "v_mul_f32 %[t1], %[q], %[t1]\n" "v_cndmask_b32 %[t1], 0, %[t1], vcc\n" "v_cvt_f64_f32 %[td], %[t1]\n"       \
                  "v_add_f64 %[a" #R "], %[a" #R "], %[td]\n" "v_add_f64 %[c" #R "], %[c" #R "], %[td]\n"
// chain Y: t0 = m, then m r, then w; t1 = r, then p_i - p_j; t2 = p_i, then p_i + p_j
#define VW_BOTH(R) "v_add_f32 %[t0], %[x" #R "], %[y]\n" "v_add_f32 %[t1], %[k" #R "], %[cj]\n" "v_mul_f32 %[t2], %[x" #R "], %[i" #R "]\n" \
                   "v_mul_f32 %[t0], %[t0], %[t1]\n" "v_cmp_lt_f32 vcc, 0, %[t1]\n" "v_rsq_f32 %[t0], %[t0]\n" "s_nop 0\n"                \
                   "v_mul_f32 %[t0], %[l], %[t0]\n" "v_cndmask_b32 %[t0], 0, %[t0], vcc\n" "v_sub_f32 %[t1], %[t2], %[p]\n"            \
                   "v_add_f32 %[t2], %[t2], %[p]\n" "v_mul_f32 %[t1], |%[t1]|, %[t0]\n" "v_mul_f32 %[t2], %[t2], %[t0]\n"              \
                   "v_cvt_f64_f32 %[td], %[t1]\n" "v_add_f64 %[a" #R "], %[a" #R "], %[td]\n"                                           \
                   "v_cvt_f64_f32 %[td], %[t2]\n" "v_add_f64 %[c" #R "], %[c" #R "], %[td]\n"
#define VW_X(R, N) ".Lx" #R "_%=:\n" VW_ONE(R) "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc0 .Ly" #N "_%=\n"
#define VW_XLAST(R) ".Lx" #R "_%=:\n" VW_ONE(R) "s_branch .Lend_%=\n"
#define VW_Y(R, N) ".Ly" #R "_%=:\n" VW_BOTH(R) "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc1 .Lx" #N "_%=\n"
#define VW_YLAST(R) ".Ly" #R "_%=:\n" VW_BOTH(R)
#define VW_BLOCK(H) "s_cmp_eq_u32 %[x0], 0\n" "s_cbranch_scc0 .Ly0_%=\n" XW_CHAIN##H(VW_X, VW_XLAST) XW_CHAIN##H(VW_Y, VW_YLAST) ".Lend_%=:"
#define VW_ROW(R) , [x##R] "s"(x[R]), [k##R] "s"(k[R]), [T##R] "v"(T[R]), [i##R] "v"(iT[R])

// The H rows of one branch: a[], c[] = the lane's numerators and denominators; x[], k[] = the bits of the rows' x and
// c (scalar); T[], iT[] = the rows' totals and their reciprocals; y, cj, p, q = the lane's own cell; l = the length.
template <int H> struct VBranch;
#define VW_DEFINE(H)                                                                                                      \
    template <> struct VBranch<H> {                                                                                       \
        static __device__ __forceinline__ void run(double (&a)[H], double (&c)[H], const uint32_t (&x)[H],                \
                                                   const uint32_t (&k)[H], const float (&T)[H], const float (&iT)[H],     \
                                                   float y, float cj, float p, float q, float l)                          \
        {                                                                                                                 \
            float t0, t1, t2;                                                                                             \
            double td;                                                                                                    \
            asm volatile(VW_BLOCK(H) : [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [td] "=&v"(td) XW_ROWS##H(XW_ACC)    \
                         : [y] "v"(y), [cj] "v"(cj), [p] "v"(p), [q] "v"(q), [l] "v"(l) XW_ROWS##H(VW_ROW)                 \
                         : "scc", "vcc", "memory");                                                                       \
        }                                                                                                                 \
    };
VW_DEFINE(8)
VW_DEFINE(16)

// Uses a set of operands (the rows' H cells of plane A, the length, the lane's two cells) so that the compiler waits
// for them here and keeps what is requested next behind this point, as g_use does.
#define VW_DEFINE_USE(H)                                                                                       \
    __device__ __forceinline__ void vw_use(const unsigned long long (&x)[H], double l, float2 ya, float2 yb)   \
    {                                                                                                          \
        asm volatile("" : : "s"(l), "v"(ya.x), "v"(ya.y), "v"(yb.x), "v"(yb.y) XW_ROWS##H(GW_CELL) : "memory"); \
    }
VW_DEFINE_USE(8)
VW_DEFINE_USE(16)

// H x 64 tile per wave, one tile per wave, the full staged row range in order (the geometry of pair_general_kernel).
// VA / VB: the two planes, ld cells a row; VT: (T, 1 / T) per sample, padded like a row of the planes.
template <int H>
G_F32 __global__ __launch_bounds__(256)
void pair_vaw_kernel(const float2 *__restrict__ VA, const float2 *__restrict__ VB, const float2 *__restrict__ VT, int64_t ld,
                     const double *__restrict__ branch_len, int64_t n_branches, const XTile *__restrict__ tiles, int n_tiles,
                     int64_t row_begin, int64_t row_end, int64_t slot_begin, double *__restrict__ out)
{
    static_assert(H - 1 <= G_VALUES_PAD, "the last staged row is read H - 1 cells past its end");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * 4 + wave;
    if (t >= n_tiles) return;
    const XTile tile = tiles[t];
    typedef const __attribute__((address_space(4))) unsigned long long *ccell;
    typedef const __attribute__((address_space(4))) double *cdouble;
    double a[H], c[H];  // numer / denom
    float T[H], iT[H];  // (uniform: scalar loads, once per tile)
    {
        ccell pt = (ccell)(VT + tile.i0);
#pragma unroll
        for (int r = 0; r < H; ++r) {
            const unsigned long long cell = pt[r];
            T[r] = __builtin_bit_cast(float, (uint32_t)cell);
            iT[r] = __builtin_bit_cast(float, (uint32_t)(cell >> 32));
            a[r] = 0.0;
            c[r] = 0.0;
        }
    }
    const float2 *pa = VA + tile.j0 + lane, *pb = VB + tile.j0 + lane;
    ccell pi = (ccell)(VA + tile.i0);
    cdouble pl = (cdouble)branch_len;
    // Two sets of operands taken in turn, as in pair_general_kernel: branch k + 1's are requested before branch k is
    // worked on.
    unsigned long long xa[H], xb[H];
    double la, lb;
    float2 yaa, yab, yba, ybb;  // (set a / b, plane A / B)
    auto request = [&](int64_t k, unsigned long long (&x)[H], double &l, float2 &ya, float2 &yb) G_F32 {
        const int64_t kk = k < n_branches ? k : n_branches - 1;  // (one past the end: the last row again, never used)
        l = pl[kk];
        ya = pa[kk * ld];
        yb = pb[kk * ld];
#pragma unroll
        for (int r = 0; r < H; ++r) x[r] = pi[kk * ld + r];
    };
    if (n_branches > 0) {
        auto work = [&](const unsigned long long (&x)[H], double l, float2 ya, float2 yb) G_F32 {
            uint32_t xs[H], ks[H];
#pragma unroll
            for (int r = 0; r < H; ++r) {
                xs[r] = (uint32_t)x[r];
                ks[r] = (uint32_t)(x[r] >> 32);
            }
            VBranch<H>::run(a, c, xs, ks, T, iT, ya.x, ya.y, yb.x, yb.y, (float)l);
        };
        request(0, xa, la, yaa, yab);
        const int64_t n_even = n_branches & ~(int64_t)1;
        for (int64_t k = 0; k < n_even; k += 2) {
            vw_use(xa, la, yaa, yab);
            request(k + 1, xb, lb, yba, ybb);
            work(xa, la, yaa, yab);
            vw_use(xb, lb, yba, ybb);
            request(k + 2, xa, la, yaa, yab);
            work(xb, lb, yba, ybb);
        }
        if (n_even < n_branches) work(xa, la, yaa, yab);
    }
    const int64_t j = tile.j0 + lane;
#pragma unroll
    for (int r = 0; r < H; ++r) {
        const int64_t i = tile.i0 + r;
        if (i < row_begin || i >= row_end || j >= i) continue;
        out[i * (i - 1) / 2 - slot_begin + j] = a[r] / c[r];  // (0 / 0 = NaN: no branch of the pair survives)
    }
}
