// ff_kernels_low_unw.hpp -- the rare rows of a sparse table, FIXED32 UNWEIGHTED (ff_schedule.hpp LOW_*).
// A fragment of ff_dev_run.hip: included there, once, inside its anonymous namespace.
//
// unifracDistUnweighted adds a branch's length to `common` where both samples have it (frcfrc/unifrac.go:144-171): in
// the staged integers common(i, j) = sum_b k_b [i has b][j has b], and U = W_i + W_j - 2 common.  On the matrix cores
// every staged row is multiplied against every pair; for a row few samples reach, "add k_r to every pair of samples that
// both have row r" is n_r^2 / 2 additions whatever the number of pairs.  Such rows stay out of the presence bits and the
// digit planes (stage_for_mfma), W keeps them, and this kernel leaves common_low(i, j) in mlow[] before the matrix-core
// kernel runs; every exit of that path takes 2 mlow off U (finish_pair, ff_kernels_finish_pair.hpp).  The same
// integers, so the distances are the unsplit path's bit for bit (tests/test_gpu_unw_split.py).
//
// What is pair_low_kernel's (ff_kernels_low.hpp, where the measurements behind each choice are): a workgroup owns a
// T x T block of pairs -- sample blocks bi, bj <= bi -- with its uint32 sums in LDS, row li at li * LOW_STRIDE words; a
// wave ANDs the two blocks' row bitmaps a word per lane, takes the rows word by word where the words are dense and 64
// rows compacted from up to 64 words where they are sparse; the lanes are dealt to the rows' B ENTRIES without gaps by a
// search over the scanned list lengths, and a round's operands are fetched while the round before is worked; every
// slot of the block is written once, zeros included (no memset, no global atomics); the diagonal block is compiled
// apart.  That part of the code is kept as a copy, so that the weighted kernel's measured code does not move.
//
// What is this kernel's own:
//   * An entry carries no value: it is the sample's place in its block, 7 bits, staged as the BYTE offset of its
//     accumulator row (li << LOW_ROW_SHIFT, at most 127 * 512 = 65,024: 16 bits).  An update's LDS address is still one
//     OR -- A's entry | B's entry >> LOW_COL_SHIFT -- and a 16-byte load brings EIGHT A entries (LowQuad: four in 32).
//   * k_r is read once per row, by the lane that looks the row up, beside the row's list bounds, and reaches the lanes
//     of the row's B entries by the shuffle that hands them a0 / na.  It keeps its whole integer length (up to 2^31):
//     no digits, no graded pieces.  The sums stay below 2^32 because common(i, j) <= W_i < 2^31.
//   * An update is one ds_add_u32 of that value: no min, no compare on values, no second operand.
//   * Loading ahead: ONE 16-byte load per step of LOW_UNW_LOAD = 8 A entries, none beyond it.  Where the split is taken
//     a rare row has a handful of entries in a block of 64 .. 128 samples (at 1 % leaf density the lists of C5's tree
//     average under three entries, at 0.2 % barely more than one), so one load IS the row's whole A list in all but a few
//     rounds, and a second load in flight would fetch another row's entries most of the time.  The latency that is
//     left is covered as in pair_low_kernel: 16 waves per workgroup, two workgroups per CU, and the next round's B entry
//     and shuffles issued before this round's adds.
//   * The tail is closed by adding ZERO, not by a branch or by the exec mask: entry u of a step is live while u < the
//     entries left, else its value is 0 and its address is whatever the load brought -- another row's entry of a block
//     of the same side (a valid accumulator row), or one of the LOW_UNW_SPARE zeros behind the array.  A step is eight
//     adds with no branch between them; the unaligned 16-byte load needs only the entries' own 2-byte alignment.
struct __attribute__((packed, aligned(2))) LowOct { uint16_t e[LOW_UNW_LOAD]; };
static_assert(sizeof(LowOct) == 16, "a step of pair_low_unw_kernel is one 16-byte load");
static_assert((127 << LOW_ROW_SHIFT) < 65536, "an entry of pair_low_unw_kernel is its accumulator row's byte offset in 16 bits");

// One B entry (this lane's: bx, col = the accumulators' column of its sample) against a row's A entries, eight per load.
// DIAGONAL: the block of pairs lies on the diagonal, each pair once -- the other half adds zero (not written out anyway).
template <bool DIAGONAL>
__device__ __forceinline__ void low_unw_walk_row(const uint16_t *__restrict__ a, uint32_t rna, uint32_t k, uint32_t bx, char *col)
{
    for (uint32_t t = 0; t < rna; t += LOW_UNW_LOAD) {
        const LowOct e = *(const LowOct *)(a + t);
        const uint32_t left = rna - t;
#pragma unroll
        for (int u = 0; u < LOW_UNW_LOAD; ++u) {
            const uint32_t ax = e.e[u];
            uint32_t v = k;
            if (u > 0) v = left > (uint32_t)u ? v : 0u;
            if (DIAGONAL) v = bx < ax ? v : 0u;
            atomicAdd((uint32_t *)(col + ax), v);
        }
    }
}
struct LowUnwRound { uint32_t ra0, rna, k, bx; bool on; };  // a lane's part of a round: its row's A list and length, its B entry, whether it has one

template <int LOW_TILE>
__global__ __launch_bounds__(LOW_THREADS)
void pair_low_unw_kernel(const uint32_t *__restrict__ ptr, const uint16_t *__restrict__ entries, const uint32_t *__restrict__ klow,
                         const unsigned long long *__restrict__ bits, int64_t words,
                         int64_t rows1, const LowTile *__restrict__ tiles, int64_t n_samples, int64_t row_begin, int64_t row_end,
                         int64_t slot_begin, uint32_t *__restrict__ mlow)
{
    __shared__ uint32_t acc[LOW_TILE * LOW_STRIDE];  // 64 / 48 / 32 KiB: row li at li * LOW_STRIDE words
    const LowTile tile = tiles[blockIdx.x];
    const int bi = tile.bi, bj = tile.bj;
    for (int q = threadIdx.x; q < LOW_TILE * LOW_STRIDE; q += LOW_THREADS) acc[q] = 0u;
    __syncthreads();
    const unsigned long long *wi = bits + (int64_t)bi * words, *wj = bits + (int64_t)bj * words;
    const uint32_t *pi = ptr + (int64_t)bi * rows1, *pj = ptr + (int64_t)bj * rows1;
    const uint32_t i_base = (uint32_t)bi * LOW_TILE, j_base = (uint32_t)bj * LOW_TILE;
    const bool diagonal = bi == bj;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int WAVES = LOW_THREADS / 64;
    // (the words of a wave, boustrophedon over the groups of 16: pair_low_kernel)
    auto word_of = [&](int64_t g) { return WAVES * g + ((g & 1) ? WAVES - 1 - wave : wave); };
    for (int64_t chunk = 0;; ++chunk) {
        const int64_t my_word = word_of(64 * chunk + lane);
        const uint32_t n_words = (uint32_t)__builtin_popcountll(__ballot(my_word < words));  // (a prefix of the lanes)
        if (n_words == 0) break;
        const unsigned long long cw = my_word < words ? wi[my_word] & wj[my_word] : 0ull;
        const uint32_t pc = (uint32_t)__builtin_popcountll(cw);
        uint32_t incl_pc = pc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl_pc, d, 64);
            if (lane >= d) incl_pc += up;
        }
        const uint32_t rows_here = (uint32_t)__builtin_amdgcn_readlane((int)incl_pc, 63);  // (a scalar: what follows is uniform)
        if (rows_here == 0) continue;
        const bool dense = rows_here >= 32u * n_words;                                   // (uniform)
        const uint32_t trips = dense ? n_words : (rows_here + 63u) / 64u;
        for (uint32_t trip = 0; trip < trips; ++trip) {
        uint32_t a0 = 0, na = 0, b0 = 0, nbb = 0, kr = 0;
        {
            int64_t r = -1;
            if (dense) {
                const unsigned long long c = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cw, (int)trip) |
                                             (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cw >> 32), (int)trip) << 32;
                if (c == 0) continue;  // (uniform)
                if ((c >> lane) & 1ull) r = word_of(64 * chunk + (int64_t)trip) * 64 + lane;
            } else {
                const uint32_t k = trip * 64u + (uint32_t)lane;
                int L = 0;  // the lane whose word holds the chunk's k-th row: the number of lanes with incl_pc <= k
#pragma unroll
                for (int step = 32; step >= 1; step >>= 1) {
                    const uint32_t v = __shfl(incl_pc, L + step - 1, 64);
                    if (v <= k) L += step;
                }
                L = min(L, 63);
                uint32_t j = k - __shfl(incl_pc - pc, L, 64);  // which of that word's rows
                const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)cw, L, 64), hi = (uint32_t)__shfl((int)(uint32_t)(cw >> 32), L, 64);
                if (k < rows_here) {
                    // the j-th set bit of the word: halve the span six times
                    uint32_t x = lo, pos = 0;
                    const uint32_t in_lo = (uint32_t)__builtin_popcount(lo);
                    if (j >= in_lo) { j -= in_lo; x = hi; pos = 32; }
#pragma unroll
                    for (int width = 16; width >= 1; width >>= 1) {
                        const uint32_t below = (uint32_t)__builtin_popcount(x & ((1u << width) - 1u));
                        if (j >= below) { j -= below; x >>= width; pos += width; }
                    }
                    r = word_of(64 * chunk + (int64_t)L) * 64 + pos;
                }
            }
            if (r >= 0) {  // the row's lists in the two blocks, and its integer length: once per row
                a0 = pi[r];
                na = pi[r + 1] - a0;
                b0 = pj[r];
                nbb = pj[r + 1] - b0;
                kr = klow[r];
            }
        }
        uint32_t inclb = nbb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inclb, d, 64);
            if (lane >= d) inclb += up;
        }
        const uint32_t totalb = (uint32_t)__builtin_amdgcn_readlane((int)inclb, 63);  // (a scalar: the rounds' loop is uniform)
        const uint32_t b_at = b0 - (inclb - nbb);  // + k: the place of the rows' k-th B entry, for k in this lane's row (mod 2^32)
        auto fetch = [&](uint32_t k0) {
            LowUnwRound r;
            const uint32_t k = k0 + (uint32_t)lane;
            int L = 0;  // the lane whose row holds B entry k: the number of lanes with inclb <= k
#pragma unroll
            for (int step = 32; step >= 1; step >>= 1) {
                const uint32_t v = __shfl(inclb, L + step - 1, 64);
                if (v <= k) L += step;
            }
            L = min(L, 63);  // (lanes past the rows' last entry)
            r.on = k < totalb;
            const uint32_t at = __shfl(b_at, L, 64) + k;
            r.ra0 = __shfl(a0, L, 64), r.rna = __shfl(na, L, 64), r.k = __shfl(kr, L, 64);
            r.bx = entries[r.on ? at : 0u];
            return r;
        };
        LowUnwRound cur = fetch(0);
        for (uint32_t k0 = 0; k0 < totalb; k0 += 64) {
            LowUnwRound nxt = cur;
            if (k0 + 64 < totalb) nxt = fetch(k0 + 64);  // (uniform)
            if (cur.on) {
                char *col = (char *)acc + (cur.bx >> LOW_COL_SHIFT);
                if (diagonal) low_unw_walk_row<true>(entries + cur.ra0, cur.rna, cur.k, cur.bx, col);  // (uniform)
                else low_unw_walk_row<false>(entries + cur.ra0, cur.rna, cur.k, cur.bx, col);
            }
            cur = nxt;
        }
        }  // (trip)
    }
    __syncthreads();
    // the tile's slots: row i = i_base + li holds columns j_base .. of slot i (i - 1) / 2 + j -- contiguous in j
    for (int q = threadIdx.x; q < LOW_TILE * LOW_TILE; q += LOW_THREADS) {
        const int li = q / LOW_TILE, lj = q % LOW_TILE;
        const int64_t i = (int64_t)i_base + li, j = (int64_t)j_base + lj;
        if (i < row_begin || i >= row_end || i >= n_samples || j >= i) continue;
        mlow[i * (i - 1) / 2 - slot_begin + j] = acc[li * LOW_STRIDE + lj];
    }
}
