// ff_kernels_stage.hpp -- staging of the flat nodes into what the pair kernels read: the dense matrices (FIXED32 / EXACT64), presence
// words and bits, column sums, activity lists, branch marks.
// A fragment of ff_dev_stage.hip: included there, once, inside its anonymous namespace
// (every kernel lives in exactly one translation unit, so the kernels stay internal and need no relocatable device code).


// The staged value of one weighted flat node: floor(l_b x 2^e + u_b), u_b the branch's shared offset (ff_dither.hpp).
__device__ __forceinline__ uint32_t stage_q_weighted(double len, double x_abnd, int e, int32_t b)
{
    const double x = len * x_abnd;  // treeDists[id] * abnd (unifrac.go:180)
    return (uint32_t)(unsigned long long)floor(ldexp(x, e) + ff::branch_dither(b));
}

// Stage FIXED32: one workgroup per sample scatters its flat nodes into column s.
// Weighted values are rounded with the branch's shared offset (ff_dither.hpp): q = floor(v + u_b).
__global__ void stage_fixed32_kernel(const int64_t *__restrict__ indptr,
                                     const int32_t *__restrict__ branch_id,
                                     const double *__restrict__ abnd,
                                     const double *__restrict__ branch_len,
                                     const uint32_t *__restrict__ klen, int weighted, int e,
                                     const int32_t *__restrict__ row_of,  // branch id -> staged row (null: identity)
                                     uint32_t *__restrict__ QT, int64_t ld)
{
    const int64_t s = blockIdx.x;
    const int64_t b0 = indptr[s], b1 = indptr[s + 1];
    for (int64_t t = b0 + threadIdx.x; t < b1; t += blockDim.x) {
        const int32_t b = branch_id[t];
        const int64_t row = row_of ? row_of[b] : b;
        if (row < 0) continue;  // (a rare row of a sparse table: it lives in the lists of pair_low_kernel)
        uint32_t q;
        if (weighted) {
            q = stage_q_weighted(branch_len[b], abnd[t], e, b);
        } else {
            q = klen[b];
        }
        QT[row * ld + s] = q;
    }
}

// The binary64 side of a FIXED32 distance: wex_s = sum_b l_b * x_s(b) (weighted: the sample's share
// of every denominator, unifrac.go:181,187,192) or sum_b l_b over its flat nodes (unweighted:
// result + common = (wex_i + wex_j + result) / 2).  One workgroup per sample; a fixed tree of
// additions, so the value does not depend on the launch.  Only the integer NUMERATOR carries the
// staging's rounding; the denominator comes from here (finish_fixed32_kernel).
__global__ __launch_bounds__(256)
void exact_weight_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                         const double *__restrict__ abnd, const double *__restrict__ branch_len,
                         int weighted, double *__restrict__ wex)
{
    __shared__ double part[256];
    const int64_t s = blockIdx.x;
    double acc = 0.0;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += 256)
        acc += branch_len[branch_id[t]] * (weighted ? abnd[t] : 1.0);
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) wex[s] = part[0];
}

// Branch compaction: which branches carry a flat node of any sample.
__global__ void mark_branches_kernel(const int32_t *__restrict__ branch_id, int64_t nnz, unsigned char *__restrict__ mark)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x)
        mark[branch_id[t]] = 1;
}

// Stage EXACT64: the abundance itself (weighted) or 1.0 for presence (unweighted).
__global__ void stage_exact64_kernel(const int64_t *__restrict__ indptr,
                                     const int32_t *__restrict__ branch_id,
                                     const double *__restrict__ abnd, int weighted,
                                     const int32_t *__restrict__ row_of, double *__restrict__ DT, int64_t ld)
{
    const int64_t s = blockIdx.x;
    const int64_t b0 = indptr[s], b1 = indptr[s + 1];
    for (int64_t t = b0 + threadIdx.x; t < b1; t += blockDim.x) {
        const int32_t b = branch_id[t];
        DT[(int64_t)(row_of ? row_of[b] : b) * ld + s] = weighted ? abnd[t] : 1.0;
    }
}

// Stage generalized UniFrac (pair_general_kernel): per flat node the cell (x, p), x = the abundance rounded once to
// binary32, p = l * x^alpha -- the whole term of a pair in which only this sample has the branch -- evaluated in
// binary64 and rounded once (alpha = 0: l itself).  A positive x under the smallest normal binary32 number is staged
// as that number: the kernel's reciprocal, square root and logarithm instructions take no denormals, and presence is
// what an abundance that small amounts to.
__device__ __forceinline__ float2 general_cell(double x, double l, double alpha)
{
    const double p = alpha == 0.0 ? l : l * pow(x, alpha);
    return make_float2(fmaxf((float)x, 1.17549435e-38f), (float)p);
}
// (a split plan's row_of holds -1 for a rare branch: its cells are the rare rows' entries, low_fill_general_kernel)
__global__ void stage_general_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                                     const double *__restrict__ abnd, const double *__restrict__ branch_len, double alpha,
                                     const int32_t *__restrict__ row_of, float2 *__restrict__ GT, int64_t ld)
{
    const int64_t s = blockIdx.x;
    const int64_t b0 = indptr[s], b1 = indptr[s + 1];
    for (int64_t t = b0 + threadIdx.x; t < b1; t += blockDim.x) {
        const int32_t b = branch_id[t];
        const double x = abnd[t], l = branch_len[b];
        if (!(x > 0.0)) continue;  // (a flat node without abundance: the sample has not the branch)
        const int64_t r = row_of ? row_of[b] : b;
        if (r < 0) continue;
        GT[r * ld + s] = general_cell(x, l, alpha);
    }
}

// The samples' totals of the staged one-sided terms over ALL rows, T_s = sum_b (binary32 p_s(b)), in binary64 by a fixed
// tree of additions (the scale of gfix and the test that declines a split come from them: not from the launch).  One
// workgroup per sample.
__global__ __launch_bounds__(256)
void general_totals_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id, const double *__restrict__ abnd,
                           const double *__restrict__ branch_len, double alpha, double *__restrict__ total)
{
    __shared__ double part[256];
    const int64_t s = blockIdx.x;
    double mine = 0.0;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x)
        if (abnd[t] > 0.0) mine += (double)general_cell(abnd[t], branch_len[branch_id[t]], alpha).y;
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[s] = part[0];
}

// Stage variance-adjusted weighted UniFrac (pair_vaw_kernel, ff_kernels_vaw.hpp), three kernels.
// (1) vaw_totals_kernel, a block per sample: T_s = the largest abundance of the list (the root's subtree sum; 0 for an
// empty sample), and the largest T of the table (non-negative binary64 numbers order as their bits do).
__global__ __launch_bounds__(256)
void vaw_totals_kernel(const int64_t *__restrict__ indptr, const double *__restrict__ abnd, double *__restrict__ T,
                       unsigned long long *__restrict__ t_max)
{
    __shared__ double part[256];
    const int64_t s = blockIdx.x;
    double m = 0.0;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) m = fmax(m, abnd[t]);
    part[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        T[s] = part[0];
        atomicMax(t_max, (unsigned long long)__double_as_longlong(part[0]));
    }
}

// A non-zero staged abundance, scaled, as a NORMAL binary32 number that leaves the product m r room (2^-60 at least).
__device__ __forceinline__ double vaw_floor(double v) { return v > 0.0 ? fmax(v, 0x1p-60) : 0.0; }

// (2) stage_vaw_fill_kernel, grid (columns / 256, row chunks): per sample (T, 1 / T), scaled by `scale` (one power of
// two for the whole table), and c = T in EVERY cell of the sample's column of plane A -- what c is where the sample
// has not the branch.  The columns behind the last sample and plane B stay zero.
__global__ void stage_vaw_fill_kernel(const double *__restrict__ T, double scale, int64_t n_samples, int64_t rows,
                                      int64_t rows_per_block, float2 *__restrict__ VA, float2 *__restrict__ VT, int64_t ld)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_samples) return;
    const double t = vaw_floor(T[s] * scale);
    const float2 cell = make_float2(0.0f, (float)t);
    if (blockIdx.y == 0) VT[s] = make_float2((float)t, t > 0.0 ? (float)(1.0 / t) : 0.0f);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    for (int64_t r = r0; r < r1; ++r) VA[r * ld + s] = cell;
}

// (3) stage_vaw_kernel, a block per sample: per flat node the cells (x, c) and (p, q).  x, c = T - x (exactly 0 where
// x == T) and q = l (x / T) / sqrt(x) -- the column's part of a term in which only this sample has the branch -- are
// evaluated in binary64 and rounded once; p is the BINARY32 product x (1 / T) of the staged numbers, the operation by
// which the kernel forms the p of its rows: equal lists give equal bits on both sides of a pair.
__global__ void stage_vaw_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                                 const double *__restrict__ abnd, const double *__restrict__ branch_len,
                                 const double *__restrict__ T, double scale, const int32_t *__restrict__ row_of,
                                 float2 *__restrict__ VA, float2 *__restrict__ VB, const float2 *__restrict__ VT, int64_t ld)
{
    const int64_t s = blockIdx.x;
    const int64_t b0 = indptr[s], b1 = indptr[s + 1];
    const double tot = T[s];
    const float inv_t = VT[s].y;
    for (int64_t t = b0 + threadIdx.x; t < b1; t += blockDim.x) {
        const int32_t b = branch_id[t];
        const double x = abnd[t], l = branch_len[b];
        if (!(x > 0.0)) continue;  // (a flat node without abundance: the sample has not the branch)
        const double xs = vaw_floor(x * scale);
        const float xf = (float)xs;
        const double q = l * (x / tot) / sqrt(xs);
        const int64_t at = (int64_t)(row_of ? row_of[b] : b) * ld + s;
        VA[at] = make_float2(xf, (float)vaw_floor((tot - x) * scale));
        VB[at] = make_float2(__fmul_rn(xf, inv_t), q > 0.0 ? fmaxf((float)q, 1.17549435e-38f) : 0.0f);
    }
}

// (4) stage_vaw_bits_kernel, a block per sample, for pair_vaw_skip_kernel (ff_kernels_vaw_skip.hpp): bit (row % XU_SLAB) of
// word [row / XU_SLAB][s] where stage_vaw_kernel wrote a cell with x != 0 -- the same test of the same flat node.  The
// occupancy words per row group and per column group are xu_occupancy_kernel's over these words.
__global__ void stage_vaw_bits_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                                      const double *__restrict__ abnd, const int32_t *__restrict__ row_of,
                                      uint32_t *__restrict__ Xb, int64_t ldx)
{
    const int64_t s = blockIdx.x;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) {
        if (!(abnd[t] > 0.0)) continue;
        const int32_t b = branch_id[t], row = row_of ? row_of[b] : b;
        atomicOr(&Xb[(int64_t)(row / XU_SLAB) * ldx + s], 1u << (row % XU_SLAB));
    }
}

// W_s = sum_b q_s(b): grid (ld/64, row chunks), one column per lane.
__global__ void colsum_kernel(const uint32_t *__restrict__ QT, int64_t ld, int64_t rows,
                              int64_t rows_per_block, unsigned long long *__restrict__ W)
{
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = min(rows, r0 + rows_per_block);
    unsigned long long acc = 0;
    for (int64_t r = r0; r < r1; ++r) acc += QT[r * ld + s];
    if (acc) atomicAdd(&W[s], acc);
}

// cs16[t][s] = sum of column s over the rows [0, 16 t).  Three launches over chunks of PFX_CHUNK_ROWS rows -- the
// chunks' sums, their exclusive scan per column, the marks of every chunk from its base -- so that a column is walked
// by rows / PFX_CHUNK_ROWS threads instead of one (one thread per column took 38 ms for C5's 100,000 rows: more than
// a pass of the kernel the sums are for; two reads of the staged matrix at the memory's rate take 2).
constexpr int PFX_CHUNK_ROWS = 1024;  // a multiple of 16
__global__ void prefix16_sums_kernel(const uint32_t *__restrict__ QT, int64_t ld, int64_t rows,
                                     uint32_t *__restrict__ chunk_sums)  // [chunk][ld]
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ld) return;
    const int64_t r0 = (int64_t)blockIdx.y * PFX_CHUNK_ROWS, r1 = min(rows, r0 + PFX_CHUNK_ROWS);
    uint32_t run = 0;
    for (int64_t r = r0; r < r1; ++r) run += QT[r * ld + s];
    chunk_sums[(int64_t)blockIdx.y * ld + s] = run;
}

__global__ void prefix16_scan_kernel(uint32_t *__restrict__ chunk_sums, int64_t ld, int64_t n_chunks)  // -> exclusive, in place
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ld) return;
    uint32_t run = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const uint32_t v = chunk_sums[c * ld + s];
        chunk_sums[c * ld + s] = run;
        run += v;
    }
}

__global__ void prefix16_fill_kernel(const uint32_t *__restrict__ QT, int64_t ld, int64_t rows,
                                     const uint32_t *__restrict__ chunk_base, uint32_t *__restrict__ cs16)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ld) return;
    const int64_t r0 = (int64_t)blockIdx.y * PFX_CHUNK_ROWS, r1 = min(rows, r0 + PFX_CHUNK_ROWS);
    uint32_t run = chunk_base[(int64_t)blockIdx.y * ld + s];
    if (blockIdx.y == 0) cs16[s] = 0;
    for (int64_t r = r0; r < r1; ++r) {
        run += QT[r * ld + s];
        if ((r & 15) == 15) cs16[((r >> 4) + 1) * ld + s] = run;
    }
}

// act64[iblock][w] bit r: branch row 64 w + r has a non-zero value among the 32 samples of
// i-block `iblock`.  One wave per (i-block, 64 rows), lane = row.
__global__ void build_activity_kernel(const uint32_t *__restrict__ QT, int64_t ld, int64_t rows, int64_t words,
                                      unsigned long long *__restrict__ act64)
{
    const int64_t w = blockIdx.x, iblock = blockIdx.y;
    const int64_t row = w * 64 + threadIdx.x;
    uint32_t any = 0;
    if (row < rows) {
        const uint4 *p = (const uint4 *)(QT + row * ld + iblock * TILE_I);
#pragma unroll
        for (int q = 0; q < TILE_I / 4; ++q) {
            const uint4 t = p[q];
            any |= t.x | t.y | t.z | t.w;
        }
    }
    const unsigned long long mask = __ballot(any != 0);
    if (threadIdx.x == 0) act64[iblock * words + w] = mask;
}

// Presence bits from the flat nodes: one workgroup per sample builds the sample's bitmap in LDS,
// 65,536 branch rows at a time, and stores it slab by slab.  Also W_s = sum of the sample's
// integer branch lengths (what colsum_kernel gives the SAD path).
__global__ __launch_bounds__(256)
void stage_mfma_bits_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                            const uint32_t *__restrict__ klen, const int32_t *__restrict__ row_of,
                            const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ row_list,
                            unsigned long long *__restrict__ Pbits, int64_t n8, int64_t n_slabs,
                            unsigned long long *__restrict__ W)
{
    // a branch's staged rows: row_list[row_ptr[b] .. row_ptr[b + 1]) (graded staging: one or more, anywhere), else
    // the one row row_of[b], else row b
    __shared__ uint32_t bm[2048];
    const int64_t s = blockIdx.x;
    const int64_t t0 = indptr[s], t1 = indptr[s + 1];
    unsigned long long w = 0;
    for (int64_t win = 0; win * 1024 < n_slabs; ++win) {
        for (int q = threadIdx.x; q < 2048; q += 256) bm[q] = 0;
        __syncthreads();
        for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
            const int32_t b0 = branch_id[t];
            if (row_ptr) {
                for (int32_t p = row_ptr[b0]; p < row_ptr[b0 + 1]; ++p) {
                    const int64_t r = row_list[p];
                    if ((r >> 16) == win) atomicOr(&bm[(r & 65535) >> 5], 1u << (r & 31));
                }
                if (win == 0) w += klen[b0];
                continue;
            }
            const int64_t r = row_of ? row_of[b0] : b0;
            if ((r >> 16) == win) {
                atomicOr(&bm[(r & 65535) >> 5], 1u << (r & 31));
                w += klen[b0];
            }
        }
        __syncthreads();
        for (int64_t q = threadIdx.x; q < 1024 && win * 1024 + q < n_slabs; q += 256)
            Pbits[(((win * 1024 + q) >> 1) * n8 + s) * 2 + (q & 1)] =
                (unsigned long long)bm[2 * q] | ((unsigned long long)bm[2 * q + 1] << 32);
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, 64);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&W[s], w);
}

// Stage the presence bits of pair_exact_unw_kernel (ff_kernels_exact_unw.hpp): one workgroup per sample ORs bit (row & 31) into word [row / 32][s].
__global__ void stage_xbits_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                                   const int32_t *__restrict__ row_of,  // branch id -> staged row (null: identity)
                                   uint32_t *__restrict__ Xb, int64_t ldx)
{
    const int64_t s = blockIdx.x;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) {
        const int32_t b = branch_id[t], row = row_of ? row_of[b] : b;
        atomicOr(&Xb[(int64_t)(row / XU_SLAB) * ldx + s], 1u << (row % XU_SLAB));
    }
}

// The group-occupancy words of pair_exact_unw_skip_kernel from the presence bits: a wave per (64-sample column group,
// slab) ORs its 64 words -- by row groups of XU_TILE_H samples, then all of them -- into rowocc[row group][slab] and
// colocc[column group][slab] (group-major, `stride` words per group; the words behind the last slab stay zero).
__global__ __launch_bounds__(64)
void xu_occupancy_kernel(const uint32_t *__restrict__ Xb, int64_t ldx, int64_t stride, uint32_t *__restrict__ rowocc,
                         uint32_t *__restrict__ colocc)
{
    const int64_t s = blockIdx.x, g = blockIdx.y;
    const int lane = threadIdx.x;
    uint32_t w = Xb[s * ldx + g * 64 + lane];
    for (int off = 1; off < XU_TILE_H; off <<= 1) w |= __shfl_xor(w, off, 64);
    if (lane % XU_TILE_H == 0) rowocc[(g * (64 / XU_TILE_H) + lane / XU_TILE_H) * stride + s] = w;
    for (int off = XU_TILE_H; off < 64; off <<= 1) w |= __shfl_xor(w, off, 64);
    if (lane == 0) colocc[g * stride + s] = w;
}


// ---- rare rows of a sparse table: lists by sample block for pair_low_kernel (ff_schedule.hpp LOW_*) ----------------
// Layout: BLOCK-major.  ptr[block][r] .. ptr[block][r + 1] are the entries (sample, staged value) of rare row r among the
// `tile` samples of the block (rows1 = rare rows + 1 positions per block); the entries of a block are contiguous and
// ascend with the row, so a workgroup that joins two blocks streams two lists.  (Row-major -- ptr[r][block] -- was
// built first: every row of every tile cost four cache lines for a few bytes, 75 GB of fabric traffic at 1 % density.)

// Flat nodes per staged row.
__global__ void row_counts_kernel(const int32_t *__restrict__ branch_id, int64_t nnz, const int32_t *__restrict__ row_of,
                                  int32_t *__restrict__ counts)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&counts[row_of ? row_of[branch_id[t]] : branch_id[t]], 1);
}

// cnt == null: Wl[s] = sum of the staged values of sample s on its rare rows, and the same added into W[s] (which
// holds the column sums of the dense part).  cnt != null: only cnt[block of s][r] += 1 for each of them.  One
// workgroup per sample.
__global__ __launch_bounds__(256)
void low_sums_counts_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                            const double *__restrict__ abnd, const double *__restrict__ branch_len, int e,
                            const int32_t *__restrict__ low_of, int64_t rows1, int tile, uint32_t *__restrict__ cnt,
                            uint32_t *__restrict__ Wl, unsigned long long *__restrict__ W)
{
    __shared__ unsigned long long total;
    const int64_t s = blockIdx.x;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) {
        const int32_t b = branch_id[t], r = low_of[b];
        if (r < 0) continue;
        if (cnt) atomicAdd(&cnt[(s / tile) * rows1 + r], 1u);
        else mine += stage_q_weighted(branch_len[b], abnd[t], e, b);
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0 && !cnt) {
        Wl[s] = (uint32_t)total;  // (< 2^31 whenever the staging is accepted: the caller checks W)
        W[s] += total;
    }
}

// Segment blockIdx.x of `in` (n values at in + blockIdx.x * stride) -> its exclusive prefix sums in place, the
// segment's total into totals[blockIdx.x].  One workgroup per segment.
__global__ __launch_bounds__(1024)
void scan_segments_kernel(uint32_t *__restrict__ data, int64_t n, int64_t stride, uint32_t *__restrict__ totals)
{
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t carry_s;
    uint32_t *seg = data + (int64_t)blockIdx.x * stride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < n; b0 += 1024) {
        const int64_t k = b0 + threadIdx.x;
        const uint32_t v = k < n ? seg[k] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        uint32_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_tot[w];
        if (k < n) seg[k] = before + (inc - v);
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry_s;
}

// ptr[block][k] += base[block] (k <= rows: the last position of a block is its end = the next block's begin).
__global__ void low_add_base_kernel(uint32_t *__restrict__ ptr, int64_t rows1, int n_blocks, const uint32_t *__restrict__ base)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows1 * n_blocks) return;
    ptr[q] += base[q / rows1];
}

// The entries: (sample's index within its block, staged value) of every rare flat node -- 8 bytes, one load -- at
// ptr[block][r] + its turn (the order within a row's block does not matter: integer sums).  cursor: zeroed, same shape
// as ptr.
__global__ __launch_bounds__(256)
void low_fill_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                     const double *__restrict__ abnd, const double *__restrict__ branch_len, int e,
                     const int32_t *__restrict__ low_of, int64_t rows1, int tile, const uint32_t *__restrict__ ptr,
                     uint32_t *__restrict__ cursor, uint2 *__restrict__ entries)
{
    const int64_t s = blockIdx.x;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) {
        const int32_t b = branch_id[t], r = low_of[b];
        if (r < 0) continue;
        const int64_t cell = (s / tile) * rows1 + r;
        const uint32_t at = ptr[cell] + atomicAdd(&cursor[cell], 1u);
        entries[at] = uint2{(uint32_t)(s % tile) << LOW_ROW_SHIFT, stage_q_weighted(branch_len[b], abnd[t], e, b)};
    }
}

// The same for an unweighted plan (pair_low_unw_kernel): an entry is the byte offset of its sample's accumulator row
// alone, 16 bits; the row's integer length is kept by rare row, not by entry.
__global__ __launch_bounds__(256)
void low_fill_unw_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                         const int32_t *__restrict__ low_of, int64_t rows1, int tile, const uint32_t *__restrict__ ptr,
                         uint32_t *__restrict__ cursor, uint16_t *__restrict__ entries)
{
    const int64_t s = blockIdx.x;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) {
        const int32_t r = low_of[branch_id[t]];
        if (r < 0) continue;
        const int64_t cell = (s / tile) * rows1 + r;
        entries[ptr[cell] + atomicAdd(&cursor[cell], 1u)] = (uint16_t)((uint32_t)(s % tile) << LOW_ROW_SHIFT);
    }
}

// The same for a generalized plan (pair_low_general_kernel): an entry is (accumulator row's byte offset, x, q) with (x, p)
// the cell stage_general_kernel would have put into GT and q = gfix(p, e); PR[s] (zeroed) gets the sample's sum of q.
__global__ __launch_bounds__(256)
void low_fill_general_kernel(const int64_t *__restrict__ indptr, const int32_t *__restrict__ branch_id,
                             const double *__restrict__ abnd, const double *__restrict__ branch_len, double alpha, int e,
                             const int32_t *__restrict__ low_of, int64_t rows1, int tile, const uint32_t *__restrict__ ptr,
                             uint32_t *__restrict__ cursor, LowGEntry *__restrict__ entries, unsigned long long *__restrict__ PR)
{
    const int64_t s = blockIdx.x;
    for (int64_t t = indptr[s] + threadIdx.x; t < indptr[s + 1]; t += blockDim.x) {
        const int32_t b = branch_id[t], r = low_of[b];
        if (r < 0) continue;
        const int64_t cell = (s / tile) * rows1 + r;
        const float2 c = general_cell(abnd[t], branch_len[b], alpha);
        const uint64_t q = gfix(c.y, e);
        entries[ptr[cell] + atomicAdd(&cursor[cell], 1u)] = LowGEntry{(uint32_t)(s % tile) << LOW_G_ROW_SHIFT, c.x, q};
        atomicAdd(&PR[s], (unsigned long long)q);
    }
}

// bits[block][w] bit t: rare row 64 w + t has an entry in the sample block.  One wave per (word, block).
__global__ void low_bits_kernel(const uint32_t *__restrict__ ptr, int64_t n_rows, int64_t rows1, int64_t words,
                                unsigned long long *__restrict__ bits)
{
    const int64_t w = blockIdx.x, blk = blockIdx.y, r = w * 64 + threadIdx.x;
    bool any = false;
    if (r < n_rows) any = ptr[blk * rows1 + r + 1] > ptr[blk * rows1 + r];
    const unsigned long long mask = __ballot(any);
    if (threadIdx.x == 0) bits[blk * words + w] = mask;
}
