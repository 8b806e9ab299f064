// ff_kernels_vaw_skip.hpp -- the row-skipping form of pair_vaw_kernel (variance-adjusted weighted UniFrac on a sparse table).
// A fragment of ff_dev_run.hip: included there, once, inside its anonymous namespace, behind ff_kernels_vaw.hpp (whose
// chains VW_ONE / VW_BOTH, VBranch and vw_use it uses) and ff_kernels_exact_unw.hpp (xu_c128: a chunk of occupancy words).
//
// pair_vaw_kernel walks every staged row of every pair tile.  Three kinds of (tile, row) cell need less, by the dense
// kernel's own code (ff_kernels_vaw.hpp):
//   (1) NO sample of the tile has the branch: every row takes chain X with q_j = 0 and adds +0.0 to both sums.  The
//       accumulators start at +0.0 and every term is non-negative, so they never hold -0.0 and x + (+0.0) = x: leaving
//       the cell out gives the same bits.
//   (2) only the COLUMN group is empty (none of the 64 lanes has the branch, some of the H rows have): the chain-X rows
//       still add +0.0 and are left out; a chain-Y row runs with the lane's cell equal to what the staging wrote where a
//       sample has not the branch -- (x, c) = (0, T_j), (p, q) = (0, 0) -- so the two vector loads are replaced by
//       constants, T_j one register per lane loaded once per tile from VT (the binary32 number stage_vaw_fill_kernel put
//       into both places).  The same VW_BOTH on the same operand values.
//   (3) only the ROW group is empty: all H rows take chain X, which reads of the row side T[r] alone -- held in registers
//       since the prologue.  The 8 H bytes of row cells are not loaded, the row tests and branches are not run: H x VW_ONE
//       in a straight line on the lane's own two cells.
//   (4) both groups have the branch: the dense kernel's request and VBranch<H>::run, unchanged.
// The rows that remain are visited in ascending staged order, each accumulator receives the same non-zero addends in the
// same order: a pair's bits are the dense kernel's, whatever the height, the shard or the launch.
//
// Which kind a cell is comes from two scalar words per slab of XU_SLAB staged rows: the OR of the presence words of the
// tile's row group(s) (XU_TILE_H samples each; a 16-row tile ORs two, its i0 is a multiple of 8) and of its column group
// (64 samples), staged group-major and slab-minor with a zero chunk behind every stream (ff_schedule.hpp XU_OCC_* and
// VW_OCC_*; xu_occupancy_kernel over stage_vaw_bits_kernel's words).  The streams are read XU_OCC_LOAD slabs at a time by
// 16-byte scalar loads, the next chunk requested while the current one is worked on.  Per slab mr | mc == 0 reads
// nothing; otherwise the set bits of the union are walked lowest first (find-first-set, clear-lowest) and two scalar bit
// tests give the kind.  A set bit is a staged row some sample has, so every row index is below n_branches.
// Built at H = VW_SKIP_TILE_H = 8 alone: the template takes 16, but its two operand sets leave the walk no scalar
// registers (277 spills in the compiler's report).
//
// Loads ahead of use: a visited row's operands are requested when the row is FOUND, and the block of the visited row
// before it runs behind that request -- one visited row ahead, across slabs and chunks, as the dense kernel is one branch
// ahead.  Two operand sets are taken in turn (a copy from a "next" to a "current" set would wait for the loads just
// requested); only what the kind needs is requested: the length always, the lane's two cells where the column group has
// the branch, the H row cells where the row group has it.

// kind (2): chain Y alone.  A row without the branch runs only the test of the next row.
#define VS_X(R, N) ".Lx" #R "_%=:\n" "s_cmp_eq_u32 %[x" #N "], 0\n" "s_cbranch_scc0 .Ly" #N "_%=\n"
#define VS_XLAST(R) ".Lx" #R "_%=:\n" "s_branch .Lend_%=\n"
#define VS_BLOCK(H) "s_cmp_eq_u32 %[x0], 0\n" "s_cbranch_scc0 .Ly0_%=\n" XW_CHAIN##H(VS_X, VS_XLAST) XW_CHAIN##H(VW_Y, VW_YLAST) ".Lend_%=:"
#define VS_ROW(R) , [x##R] "s"(x[R]), [k##R] "s"(k[R]), [i##R] "v"(iT[R])
#define VS_T(R) , [T##R] "v"(T[R])

// The H rows of one branch where the column group is empty (VSkipY: y, cj, p are the constants 0, T_j, 0) and where the
// row group is empty (VSkipX: cj, q are the lane's own).  Operands as VBranch's.
template <int H> struct VSkipY;
template <int H> struct VSkipX;
#define VS_DEFINE(H)                                                                                                      \
    template <> struct VSkipY<H> {                                                                                        \
        static __device__ __forceinline__ void run(double (&a)[H], double (&c)[H], const uint32_t (&x)[H],                \
                                                   const uint32_t (&k)[H], const float (&iT)[H], float y, float cj,       \
                                                   float p, float l)                                                      \
        {                                                                                                                 \
            float t0, t1, t2;                                                                                             \
            double td;                                                                                                    \
            asm volatile(VS_BLOCK(H) : [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [td] "=&v"(td) XW_ROWS##H(XW_ACC)    \
                         : [y] "v"(y), [cj] "v"(cj), [p] "v"(p), [l] "v"(l) XW_ROWS##H(VS_ROW)                             \
                         : "scc", "vcc", "memory");                                                                       \
        }                                                                                                                 \
    };                                                                                                                    \
    template <> struct VSkipX<H> {                                                                                        \
        static __device__ __forceinline__ void run(double (&a)[H], double (&c)[H], const float (&T)[H], float cj, float q) \
        {                                                                                                                 \
            float t0, t1;                                                                                                 \
            double td;                                                                                                    \
            asm volatile(XW_ROWS##H(VW_ONE) : [t0] "=&v"(t0), [t1] "=&v"(t1), [td] "=&v"(td) XW_ROWS##H(XW_ACC)            \
                         : [cj] "v"(cj), [q] "v"(q) XW_ROWS##H(VS_T)                                                       \
                         : "vcc", "memory");                                                                              \
        }                                                                                                                 \
    };
VS_DEFINE(8)
static_assert(VW_SKIP_TILE_H == 8, "pair_vaw_skip_kernel: the asm blocks are spelt out at the one height it is built for");

enum : uint32_t { VS_ROWS_HAVE = 1, VS_COLS_HAVE = 2 };  // a visited row's kind: which of the tile's two groups has the branch

// pair_vaw_kernel's geometry and arguments, with the occupancy streams (n_chunks chunks of XU_OCC_LOAD slabs,
// occ_stride words per group) in place of the row count.
template <int H>
G_F32 __global__ __launch_bounds__(256)
void pair_vaw_skip_kernel(const float2 *__restrict__ VA, const float2 *__restrict__ VB, const float2 *__restrict__ VT, int64_t ld,
                          const double *__restrict__ branch_len, int n_chunks, const uint32_t *__restrict__ rowocc,
                          const uint32_t *__restrict__ colocc, int64_t occ_stride, const XTile *__restrict__ tiles, int n_tiles,
                          int64_t row_begin, int64_t row_end, int64_t slot_begin, double *__restrict__ out)
{
    static_assert(H - 1 <= G_VALUES_PAD, "the last staged row is read H - 1 cells past its end");
    static_assert(H % VW_OCC_ROW_GROUP == 0 && H / VW_OCC_ROW_GROUP <= 2, "a tile ORs the words of one or two row groups");
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
            // (kept in VECTOR registers from here on: left to itself the compiler holds the uniform values in 2 H scalar
            // registers, which the walk needs, and copies them over ahead of every block)
            asm volatile("" : "+v"(T[r]), "+v"(iT[r]));
            a[r] = 0.0;
            c[r] = 0.0;
        }
    }
    const float Tj = VT[tile.j0 + lane].x;  // the c of the lane's every cell without the branch
    const float2 *pa = VA + tile.j0 + lane, *pb = VB + tile.j0 + lane;
    ccell pi = (ccell)(VA + tile.i0);
    cdouble pl = (cdouble)branch_len;
    // (tile.i0 is a multiple of H -- build_tiles -- and H of the row groups' size: the tile's rows are whole groups)
    xu_c128 pr = (xu_c128)(rowocc + (int64_t)(tile.i0 / VW_OCC_ROW_GROUP) * occ_stride);
    xu_c128 pc = (xu_c128)(colocc + (int64_t)(tile.j0 / X_TILE_J) * occ_stride);
    const int64_t chunk_stride = occ_stride / XU_OCC_LOAD;
    auto row_masks = [&](int64_t ch) G_F32 {
        xu_u32x4 m = pr[ch];
        if (H > VW_OCC_ROW_GROUP) m |= pr[chunk_stride + ch];
        return m;
    };
    // Two sets of operands taken in turn, as in pair_vaw_kernel (the loop below names them statically: a set chosen by
    // a flag makes the compiler copy one into the other, and the copy waits for the loads just requested).
    unsigned long long xa[H], xb[H];
    double la = 0.0, lb = 0.0;
    float2 yaa = {0.0f, 0.0f}, yab = yaa, yba = yaa, ybb = yaa;  // (set a / b, plane A / B)
#pragma unroll
    for (int r = 0; r < H; ++r) xa[r] = xb[r] = 0;
    auto request = [&](int64_t row, uint32_t kind, unsigned long long (&x)[H], double &l, float2 &ya, float2 &yb) G_F32 {
        l = pl[row];
        if (kind & VS_COLS_HAVE) {
            ya = pa[row * ld];
            yb = pb[row * ld];
        }
        if (kind & VS_ROWS_HAVE) {
#pragma unroll
            for (int r = 0; r < H; ++r) x[r] = pi[row * ld + r];
        }
    };
    auto work = [&](uint32_t kind, const unsigned long long (&x)[H], double l, float2 ya, float2 yb) G_F32 {
        if (kind == VS_COLS_HAVE) {
            VSkipX<H>::run(a, c, T, ya.y, yb.y);
        } else {
            uint32_t xs[H], ks[H];
#pragma unroll
            for (int r = 0; r < H; ++r) {
                xs[r] = (uint32_t)x[r];
                ks[r] = (uint32_t)(x[r] >> 32);
            }
            if (kind == VS_ROWS_HAVE) VSkipY<H>::run(a, c, xs, ks, iT, 0.0f, Tj, 0.0f, (float)l);
            else VBranch<H>::run(a, c, xs, ks, T, iT, ya.x, ya.y, yb.x, yb.y, (float)l);
        }
    };
    // The walk: the next visited row and its kind (0: the streams are at their end; not called again after that).  The
    // current chunk's words are shifted out slab by slab; the chunk behind it is requested when the current one is taken
    // up (chunk n_chunks is the zero chunk, and n_chunks >= 1).
    xu_u32x4 mr4 = row_masks(0), mc4 = pc[0], mr4n = row_masks(1), mc4n = pc[1];
    int ch = 0, q = -1;
    uint32_t m = 0, mr = 0, mc = 0;
    auto next = [&](int64_t &row) G_F32 -> uint32_t {
        while (m == 0) {
            if (++q == XU_OCC_LOAD) {
                if (++ch >= n_chunks) return 0;
                q = 0;
                mr4 = mr4n;
                mc4 = mc4n;
                mr4n = row_masks((int64_t)ch + 1);
                mc4n = pc[(int64_t)ch + 1];
            }
            mr = mr4[0];
            mc = mc4[0];
            mr4 = xu_u32x4{mr4[1], mr4[2], mr4[3], 0u};
            mc4 = xu_u32x4{mc4[1], mc4[2], mc4[3], 0u};
            m = mr | mc;
        }
        const uint32_t k = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        row = ((int64_t)ch * XU_OCC_LOAD + q) * XU_SLAB + k;
        return ((mr >> k) & 1u) * VS_ROWS_HAVE | ((mc >> k) & 1u) * VS_COLS_HAVE;
    };
    int64_t row = 0;
    uint32_t ka = next(row), kb = 0;
    if (ka) {
        request(row, ka, xa, la, yaa, yab);
        for (;;) {
            kb = next(row);
            vw_use(xa, la, yaa, yab);
            if (kb) request(row, kb, xb, lb, yba, ybb);
            work(ka, xa, la, yaa, yab);
            if (!kb) break;
            ka = next(row);
            vw_use(xb, lb, yba, ybb);
            if (ka) request(row, ka, xa, la, yaa, yab);
            work(kb, xb, lb, yba, ybb);
            if (!ka) break;
        }
    }
    const int64_t j = tile.j0 + lane;
#pragma unroll
    for (int r = 0; r < H; ++r) {
        const int64_t i = tile.i0 + r;
        if (i < row_begin || i >= row_end || j >= i) continue;
        out[i * (i - 1) / 2 - slot_begin + j] = a[r] / c[r];  // (0 / 0 = NaN: no branch of the pair survives)
    }
}

// What the skipping form does on the shard's tiles, counted exactly from the occupancy words and the presence words
// (Xb[slab][sample], ldx words a slab): the visited (tile, row) cells by kind, the (tile, slab) cells that are not empty,
// and the chain-Y rows that run in the cells whose column group is empty.  A wave per tile; h = the tiles' height.
enum { VS_CNT_BOTH = 0, VS_CNT_COL_EMPTY = 1, VS_CNT_ROW_EMPTY = 2, VS_CNT_SLABS = 3, VS_CNT_Y_ROWS = 4, VS_CNT_N = 5 };
__global__ __launch_bounds__(64)
void vw_visit_count_kernel(const XTile *__restrict__ tiles, int h, const uint32_t *__restrict__ rowocc, const uint32_t *__restrict__ colocc,
                           int64_t occ_stride, const uint32_t *__restrict__ Xb, int64_t ldx, int n_slabs,
                           unsigned long long *__restrict__ counts)
{
    const XTile tile = tiles[blockIdx.x];
    const uint32_t *pr = rowocc + (int64_t)(tile.i0 / VW_OCC_ROW_GROUP) * occ_stride, *pc = colocc + (int64_t)(tile.j0 / X_TILE_J) * occ_stride;
    uint32_t n[VS_CNT_N] = {0, 0, 0, 0, 0};
    for (int s = threadIdx.x; s < n_slabs; s += 64) {
        uint32_t mr = pr[s];
        if (h > VW_OCC_ROW_GROUP) mr |= pr[occ_stride + s];
        const uint32_t mc = pc[s];
        n[VS_CNT_BOTH] += (uint32_t)__popc(mr & mc);
        n[VS_CNT_COL_EMPTY] += (uint32_t)__popc(mr & ~mc);
        n[VS_CNT_ROW_EMPTY] += (uint32_t)__popc(mc & ~mr);
        n[VS_CNT_SLABS] += (mr | mc) != 0;
        if (mr & ~mc)
            for (int r = 0; r < h; ++r) n[VS_CNT_Y_ROWS] += (uint32_t)__popc(Xb[(int64_t)s * ldx + tile.i0 + r] & ~mc);
    }
#pragma unroll
    for (int q = 0; q < VS_CNT_N; ++q) {
        for (int off = 32; off > 0; off >>= 1) n[q] += __shfl_down(n[q], off, 64);
        if (threadIdx.x == 0 && n[q]) atomicAdd(&counts[q], (unsigned long long)n[q]);
    }
}
