// ff_kernels_general.hpp -- generalized UniFrac d(alpha) (Chen et al. 2012), alpha != 1: binary32 terms, binary64 sums.
// A fragment of ff_dev_run.hip: included there, once, inside its anonymous namespace.
//
// With s = x_i(b) + x_j(b) and d = |x_i(b) - x_j(b)|, over the branches with s > 0,
//     numer = sum_b l_b s^alpha (d / s)        denom = sum_b l_b s^alpha        d(alpha) = numer / denom.
// Neither an L1 distance (v_sad_u32) nor a contraction (the matrix cores): every (pair, branch) term carries a power.
// But as in pair_exact64_skip_kernel (ff_kernels_exact_w.hpp) most terms are one-sided, and for those d = s: the term is
// l y^alpha in the numerator AND in the denominator -- p, a property of the column alone, computed ONCE, when the
// matrix is staged, in binary64 (stage_general_kernel).  The staged matrix GT[row][sample] holds (x, p) as two
// binary32 values; a wave owns an H x 64 pair tile, its lane one column, and per branch it takes, by the row's x -- a
// scalar --,
//     row has not the branch:   numer += p_col ;  denom += p_col                   (two binary64 additions, nothing else;
//                                                                                   absent / absent adds +0 twice)
//     row has it:               s = x + y, d = |x - y|, t = s^(alpha - 1)
//                               numer += l (d t) ;  denom += l (s t)               (a lane whose own y is 0 computes the
//                                                                                   row's one-sided term here: d == s bit
//                                                                                   for bit, the two addends are equal)
// The power is needed on 7 % of the cells at C3's density.  KIND picks t at launch, not per term:
//     G_ZERO  alpha = 0     numer += l (d * rcp(s)), denom += l          one v_rcp_f32 (d == s selects the quotient 1)
//     G_HALF  alpha = 0.5   t = rsq(s)                                   one v_rsq_f32
//     G_ANY   otherwise     t = exp2((alpha - 1) * log2(s))              v_log_f32, v_mul_f32, v_exp_f32
// The staging keeps every present x a NORMAL binary32 number (these instructions take no denormals), so s is one too.
//
// Accuracy: every term is non-negative, so the relative error of either sum is at most the largest
// relative error of a term; the sums themselves are binary64 (2^-53 per addition).  The only cancellation, d = |x - y|
// of two rounded inputs, is off by at most 2^-24 s -- 2^-24 of the matching denominator term.  With d(alpha) <= 1 the
// result is within (roundings per term + 2) 2^-24 absolute: at most 8 roundings for G_ZERO / G_HALF, 4.8e-7; G_ANY adds
// |alpha - 1| |log2 s| 2^-23 on terms that weigh s^alpha.  One-sided terms carry ONE rounding (p).
//
// Control flow: as in XwBranch (ff_kernels_exact_w.hpp) the H rows of a branch are ONE asm block in two chains, X ("the
// row before has not the branch") and Y ("it has"), each row's code ending with the test of the next row and falling
// through into its own kind: a branch instruction is taken only where consecutive rows differ.  (The same chains in
// plain C++ -- gotos between two rows of labelled blocks -- do not survive the compiler: it rebuilds the diamond per row
// and copies all 2 H accumulators at every join.)  An asm block is outside the compiler's hazard bookkeeping: gfx950
// wants one wait state between a transcendental instruction and a plain VALU instruction that reads its result; every
// v_rcp / v_rsq / v_log / v_exp below is followed by an s_nop.
//
// Both accumulators of a pair are binary64 (4 H registers), every wave walks ALL staged rows in ascending order: a
// pair's sums are the same additions in the same order whatever the tile height, the shard or the launch.

enum { G_ZERO = 0, G_HALF = 1, G_ANY = 2 };

// (The little binary32 arithmetic left to the compiler -- conversions -- is compiled without the packed binary32
// instructions.)
#define G_F32 __attribute__((target("no-packed-fp32-ops")))

// s = x + y -> t0, x - y -> t1 (its sign is dropped where it is used), then t2 = s^(alpha - 1) by KIND
#define GW_SD(R) "v_add_f32 %[t0], %[x" #R "], %[y]\n" "v_sub_f32 %[t1], %[x" #R "], %[y]\n"
// numer += l (|t1| t2), denom += l (t0 t2)
#define GW_TERMS(R) "v_mul_f32 %[t1], |%[t1]|, %[t2]\n" "v_mul_f32 %[t0], %[t0], %[t2]\n" "v_mul_f32 %[t1], %[l], %[t1]\n" \
                    "v_mul_f32 %[t0], %[l], %[t0]\n" "v_cvt_f64_f32 %[td], %[t1]\n" "v_add_f64 %[a" #R "], %[a" #R "], %[td]\n" \
                    "v_cvt_f64_f32 %[td], %[t0]\n" "v_add_f64 %[c" #R "], %[c" #R "], %[td]\n"
// G_ZERO: the quotient d / s, exactly 1 where d == s (a lane without the branch: numer and denom get the same addend)
#define GW_BOTH0(R) GW_SD(R) "v_rcp_f32 %[t2], %[t0]\n" "s_nop 0\n" "v_mul_f32 %[t2], |%[t1]|, %[t2]\n" "v_cmp_eq_f32 vcc, |%[t1]|, %[t0]\n" \
                    "v_cndmask_b32 %[t2], %[t2], 1.0, vcc\n" "v_mul_f32 %[t2], %[l], %[t2]\n" "v_cvt_f64_f32 %[td], %[t2]\n" \
                    "v_add_f64 %[a" #R "], %[a" #R "], %[td]\n" "v_add_f64 %[c" #R "], %[c" #R "], %[ld]\n"
#define GW_BOTH1(R) GW_SD(R) "v_rsq_f32 %[t2], %[t0]\n" "s_nop 0\n" GW_TERMS(R)
#define GW_BOTH2(R) GW_SD(R) "v_log_f32 %[t2], %[t0]\n" "s_nop 0\n" "v_mul_f32 %[t2], %[am1], %[t2]\n" "s_nop 0\n" "v_exp_f32 %[t2], %[t2]\n" "s_nop 0\n" GW_TERMS(R)
#define GW_X(R, N) ".Lx" #R "_%=:\n" "v_add_f64 %[a" #R "], %[a" #R "], %[p]\n" "v_add_f64 %[c" #R "], %[c" #R "], %[p]\n" \
                   "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc0 .Ly" #N "_%=\n"
#define GW_XLAST(R) ".Lx" #R "_%=:\n" "v_add_f64 %[a" #R "], %[a" #R "], %[p]\n" "v_add_f64 %[c" #R "], %[c" #R "], %[p]\n" "s_branch .Lend_%=\n"
#define GW_Y0(R, N) ".Ly" #R "_%=:\n" GW_BOTH0(R) "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc1 .Lx" #N "_%=\n"
#define GW_Y1(R, N) ".Ly" #R "_%=:\n" GW_BOTH1(R) "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc1 .Lx" #N "_%=\n"
#define GW_Y2(R, N) ".Ly" #R "_%=:\n" GW_BOTH2(R) "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc1 .Lx" #N "_%=\n"
#define GW_YLAST0(R) ".Ly" #R "_%=:\n" GW_BOTH0(R)
#define GW_YLAST1(R) ".Ly" #R "_%=:\n" GW_BOTH1(R)
#define GW_YLAST2(R) ".Ly" #R "_%=:\n" GW_BOTH2(R)
#define GW_BLOCK(K, H) "s_cmp_eq_u32 %[x0], 0\n" "s_cbranch_scc0 .Ly0_%=\n" XW_CHAIN##H(GW_X, GW_XLAST) XW_CHAIN##H(GW_Y##K, GW_YLAST##K) ".Lend_%=:"
#define GW_XS(R) , [x##R] "s"(x[R])

// The H rows of one branch: a[], c[] = the lane's numerators and denominators, x[] = the bits of the rows' values
// (scalar), y / p = the lane's column value and its one-sided term, l = the branch length in binary32 (ld: the same
// number as a binary64 addend, G_ZERO's denominator term), am1 = alpha - 1 (G_ANY).
template <int KIND, int H> struct GBranch;
#define G_DEFINE(K, H)                                                                                                        \
    template <> struct GBranch<K, H> {                                                                                        \
        static __device__ __forceinline__ void run(double (&a)[H], double (&c)[H], const uint32_t (&x)[H], float y, double p,  \
                                                   float l, double ld, float am1)                                              \
        {                                                                                                                     \
            float t0, t1, t2;                                                                                                 \
            double td;                                                                                                        \
            asm volatile(GW_BLOCK(K, H) : [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [td] "=&v"(td) XW_ROWS##H(XW_ACC)       \
                         : [y] "v"(y), [l] "v"(l), [ld] "v"(ld), [p] "v"(p), [am1] "s"(am1) XW_ROWS##H(GW_XS) : "scc", "vcc", "memory"); \
        }                                                                                                                     \
    };
G_DEFINE(0, 8)
G_DEFINE(1, 8)
G_DEFINE(2, 8)
G_DEFINE(0, 16)
G_DEFINE(1, 16)
G_DEFINE(2, 16)

// Uses a set of operands -- the rows' H cells WHOLE (x and p, 8 bytes: what keeps their loads wide; the kernel reads only
// the x halves), the length, the lane's cell -- so that the compiler waits for them here, and keeps what is requested
// next behind this point (as the empty asm statements of pair_exact64_skip_kernel do).
#define GW_CELL(R) , "s"(x[R])
#define G_DEFINE_USE(H)                                                                                            \
    __device__ __forceinline__ void g_use(const unsigned long long (&x)[H], double l, float2 y)                    \
    {                                                                                                              \
        asm volatile("" : : "s"(l), "v"(y.x), "v"(y.y) XW_ROWS##H(GW_CELL) : "memory");                            \
    }
G_DEFINE_USE(8)
G_DEFINE_USE(16)

// H x 64 tile per wave, one tile per wave, the full staged row range in order (the geometry of pair_exact64_skip_kernel).
// SPLIT: the plan keeps its rare rows out of GT (ff_kernels_low_general.hpp); glow[slot] holds their (Mn, Md), PR[s] the
// samples' quantised sums over them, and the epilogue adds (PR_i + PR_j - M) 2^-e -- an exact integer below 2^62, rounded
// once -- to either sum before the division.  Without the flag the three trailing arguments are not read: today's code.
template <int KIND, int H, bool SPLIT = false>
G_F32 __global__ __launch_bounds__(256)
void pair_general_kernel(const float2 *__restrict__ GT, int64_t ld, const double *__restrict__ branch_len, int64_t n_branches,
                         float am1, const XTile *__restrict__ tiles, int n_tiles, int64_t row_begin, int64_t row_end,
                         int64_t slot_begin, double *__restrict__ out, const ulong2 *__restrict__ glow = nullptr,
                         const unsigned long long *__restrict__ PR = nullptr, double inv_scale = 0.0)
{
    static_assert(H - 1 <= G_VALUES_PAD, "the last staged row is read H - 1 cells past its end");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = blockIdx.x * 4 + wave;
    if (t >= n_tiles) return;
    const XTile tile = tiles[t];
    double a[H], c[H];  // numer / denom
#pragma unroll
    for (int r = 0; r < H; ++r) {
        a[r] = 0.0;
        c[r] = 0.0;
    }
    // (uniform addresses: scalar loads.  A row cell is fetched whole, 8 bytes, so that the H of them are one or two
    // wide loads; only its x is used)
    typedef const __attribute__((address_space(4))) unsigned long long *ccell;
    typedef const __attribute__((address_space(4))) double *cdouble;
    const float2 *pj = GT + tile.j0 + lane;
    ccell pi = (ccell)(GT + tile.i0);
    cdouble pl = (cdouble)branch_len;
    // Two sets of operands taken in turn, as in pair_exact64_skip_kernel: branch k + 1's are requested before branch k
    // is worked on; the empty asm statements use the current set (the compiler waits there) and keep the next
    // requests behind them.
    unsigned long long xa[H], xb[H];
    double la, lb;
    float2 ya, yb;
    auto request = [&](int64_t k, unsigned long long (&x)[H], double &l, float2 &y) G_F32 {
        const int64_t kk = k < n_branches ? k : n_branches - 1;  // (one past the end: the last row again, never used)
        l = pl[kk];
        y = pj[kk * ld];
#pragma unroll
        for (int r = 0; r < H; ++r) x[r] = pi[kk * ld + r];
    };
    if (n_branches > 0) {
        auto work = [&](const unsigned long long (&x)[H], double l, float2 y) G_F32 {
            uint32_t xs[H];
#pragma unroll
            for (int r = 0; r < H; ++r) xs[r] = (uint32_t)x[r];
            const float lf = (float)l;  // (G_ZERO adds THIS length to the denominators: the addend of its numerator where d == s, and the staged p)
            GBranch<KIND, H>::run(a, c, xs, y.x, (double)y.y, lf, (double)lf, am1);
        };
        request(0, xa, la, ya);
        // (pairs of branches in ONE basic block, an odd last branch behind the loop: pair_exact64_skip_kernel says why)
        const int64_t n_even = n_branches & ~(int64_t)1;
        for (int64_t k = 0; k < n_even; k += 2) {
            g_use(xa, la, ya);
            request(k + 1, xb, lb, yb);
            work(xa, la, ya);
            g_use(xb, lb, yb);
            request(k + 2, xa, la, ya);
            work(xb, lb, yb);
        }
        if (n_even < n_branches) work(xa, la, ya);
    }
    const int64_t j = tile.j0 + lane;
#pragma unroll
    for (int r = 0; r < H; ++r) {
        const int64_t i = tile.i0 + r;
        if (i < row_begin || i >= row_end || j >= i) continue;
        if (SPLIT) {
            const ulong2 m = glow[i * (i - 1) / 2 - slot_begin + j];
            const unsigned long long both = PR[i] + PR[j];
            a[r] += (double)(both - m.x) * inv_scale;
            c[r] += (double)(both - m.y) * inv_scale;
        }
        out[i * (i - 1) / 2 - slot_begin + j] = a[r] / c[r];  // (0 / 0 = NaN: two empty samples, as unifrac.go:204)
    }
}
