// ff_kernels_low_general.hpp -- the rare rows of a sparse table, GENERALIZED UniFrac d(alpha) (ff_schedule.hpp LOW_G_*,
// DESIGN 4.14).  A fragment of ff_dev_run.hip: included there, once, inside its anonymous namespace, behind
// ff_kernels_general.hpp (whose KINDs and term arithmetic it shares).
//
// pair_general_kernel walks every staged row of every pair tile.  But a branch only ONE sample of a pair has adds the
// column's own staged term p = l x^alpha to the numerator and to the denominator, and only a branch BOTH have needs the
// pair's arithmetic.  For a set R of rows few samples reach, with P_s = sum over R of p_s(b),
//     numer_R(i, j) = P_i + P_j - sum over the rows of R both have of (p_i + p_j - l s^(alpha - 1) d)
//     denom_R(i, j) = P_i + P_j - sum over the rows of R both have of (p_i + p_j - l s^alpha)
// -- n_r^2 / 2 updates per row whatever the number of pairs.  Such rows stay out of GT and of the lengths by staged row,
// this kernel leaves the two sums over "both have" in glow[] before pair_general_kernel runs, and that kernel's
// epilogue (its SPLIT instantiation) adds P_i + P_j - M to its binary64 sums before it divides.
// (Variance-adjusted UniFrac has no such form: its one-sided term holds the OTHER sample's total, ff_kernels_vaw.hpp.)
//
// Arithmetic.  P_i + P_j - M in floating point cancels, and floating-point LDS atomics depend on their order: the rare
// rows' sums are 64-bit INTEGERS.  gfix(t, e) (ff_schedule.hpp) is the binary32 term t times 2^e, truncated; the plan
// picks e so that the largest per-sample total over ALL rows lies in [2^60, 2^61).  The staging keeps q = gfix(p) in the
// entry and PR_s = sum over R of q_s(b); per pair, modulo 2^64,
//     Mn += q_i + q_j - gfix(l d t)        Md += q_i + q_j - gfix(l s t)        s = x_i + x_j, d = |x_i - x_j|, t = s^(alpha - 1)
// with t, and the two products, formed by the instructions of pair_general_kernel's KIND in its order (G_ZERO: the
// quotient selected to 1 where d == s, the denominator term the binary32 length): a both-have term is the dense
// kernel's binary32 number.  A single update may be negative modulo 2^64; PR_i + PR_j - M is the exact integer sum of
// the pair's quantised one-sided and both-have terms, >= 0 and < 2^62.  Integer adds: a pair's value does not depend on
// order, block side, shard or launch; a twin pair has d = 0, Mn = PR_i + PR_j, distance exactly 0; an empty sample
// against another gives both sums the same addends, exactly 1; empty against empty 0 / 0 = NaN.
// The bound: every effective term is non-negative and carries the dense kernel's relative error (ff_kernels_general.hpp)
// plus at most 2^-e absolute from the truncation -- 2 (rare rows) 2^-e per sum at most, which the plan keeps under
// 2^-26 of the smallest non-empty sample's total, or it declines the split (stage_for_general): DESIGN 4.12's bound
// plus 2^-25.
//
// The frame is pair_low_kernel's (ff_kernels_low.hpp, where the measurements behind each choice are): a workgroup owns
// a 64 x 64 block of pairs -- sample blocks bi, bj <= bi -- with its (Mn, Md) in LDS, 16 bytes a pair, row li at
// li * 1024 bytes: 64 KiB; a wave ANDs the two blocks' row bitmaps a word per lane, takes the rows word by word where
// the words are dense and 64 rows compacted from up to 64 words where they are sparse; the lanes are dealt to the rows'
// B ENTRIES without gaps by a search over the scanned list lengths, and a round's operands are fetched while the round
// before is worked; each lane walks its row's A list; every slot of the block is written once.  Its own:
//   * A workgroup is ONE wave (LOW_G_THREADS, ff_schedule.hpp: with the frame's 16 waves on one block the sums were not
//     repeatable on the device, for a cause not found yet); two workgroups' accumulators share a CU's LDS.
//   * An entry is 16 bytes, one load: {accumulator-row byte offset, x, q}.  An update's LDS address is still one OR,
//     A's offset | B's offset >> LOW_G_COL_SHIFT.  The row's binary32 length is read once per row beside the list
//     bounds and reaches the lanes of the row's B entries by the shuffle that hands them a0 / na.
//   * An update is the KIND's term arithmetic, two gfix (integer: a field extract, two shifts), and two ds_add_u64 on
//     adjacent words.
//   * A step is LOW_G_LOAD entries; the tail is closed by adding ZERO: past the list's end the load brings another row's
//     entry of a block of the same side (a valid accumulator row) or one of the LOW_G_SPARE zeros behind the array.
//   * DIAGONAL (bi == bj: each pair once, the other half adds zero) is a template parameter of the KERNEL: the
//     diagonal blocks are a launch of their own, ahead of the others.

// n = l (d t), dn = l (s t) of one (A, B) pair of entries of a row of binary32 length l: pair_general_kernel's GW_BOTH,
// operation for operation.
template <int KIND>
__device__ __forceinline__ void low_g_terms(float xa, float xb, float l, float am1, float &n, float &dn)
{
    // (the builtins are the bare instructions v_rcp_f32 / v_rsq_f32 / v_log_f32 / v_exp_f32; no contraction: the
    // translation unit is built with -ffp-contract=off, and no product here is followed by a sum)
    const float s = xa + xb, d = __builtin_fabsf(xa - xb);
    if (KIND == G_ZERO) {
        float q = d * __builtin_amdgcn_rcpf(s);
        q = d == s ? 1.0f : q;
        n = l * q;
        dn = l;
    } else {
        const float t = KIND == G_HALF ? __builtin_amdgcn_rsqf(s) : __builtin_amdgcn_exp2f(am1 * __builtin_amdgcn_logf(s));
        n = l * (d * t);
        dn = l * (s * t);
    }
}

// One B entry (this lane's: eb, col = the accumulators' column of its sample) against a row's A entries, LOW_G_LOAD per step.
template <int KIND, bool DIAGONAL>
__device__ __forceinline__ void low_g_walk_row(const LowGEntry *__restrict__ a, uint32_t rna, float l, const LowGEntry eb, char *col,
                                               int e, float am1)
{
    for (uint32_t t = 0; t < rna; t += LOW_G_LOAD) {
        LowGEntry ea[LOW_G_LOAD];
#pragma unroll
        for (int u = 0; u < LOW_G_LOAD; ++u) ea[u] = a[t + u];
        const uint32_t left = rna - t;
#pragma unroll
        for (int u = 0; u < LOW_G_LOAD; ++u) {
            float n, dn;
            low_g_terms<KIND>(ea[u].x, eb.x, l, am1, n, dn);
            const uint64_t both = ea[u].q + eb.q;
            uint64_t vn = both - gfix(n, e), vd = both - gfix(dn, e);
            bool live = true;
            if (u > 0) live = left > (uint32_t)u;
            if (DIAGONAL) live = live && eb.off < ea[u].off;
            vn = live ? vn : 0ull;
            vd = live ? vd : 0ull;
            unsigned long long *m = (unsigned long long *)(col + ea[u].off);
            atomicAdd(m, (unsigned long long)vn);
            atomicAdd(m + 1, (unsigned long long)vd);
        }
    }
}
struct LowGRound { uint32_t ra0, rna; float l; LowGEntry eb; bool on; };  // a lane's part of a round: its row's A list and length, its B entry, whether it has one

template <int KIND, bool DIAGONAL>
__global__ __launch_bounds__(LOW_G_THREADS)
void pair_low_general_kernel(const uint32_t *__restrict__ ptr, const LowGEntry *__restrict__ entries, const float *__restrict__ llow,
                             const unsigned long long *__restrict__ bits, int64_t words, int64_t rows1,
                             const LowTile *__restrict__ tiles, int64_t n_samples, int64_t row_begin, int64_t row_end,
                             int64_t slot_begin, int e, float am1, ulong2 *__restrict__ glow)
{
    __shared__ ulong2 acc[LOW_G_TILE * LOW_G_TILE];  // 64 KiB: pair (li, lj) at li * 1024 + lj * 16 bytes
    const LowTile tile = tiles[blockIdx.x];
    const int bi = tile.bi, bj = tile.bj;
    for (int q = threadIdx.x; q < LOW_G_TILE * LOW_G_TILE; q += LOW_G_THREADS) acc[q] = ulong2{0ull, 0ull};
    __syncthreads();
    const unsigned long long *wi = bits + (int64_t)bi * words, *wj = bits + (int64_t)bj * words;
    const uint32_t *pi = ptr + (int64_t)bi * rows1, *pj = ptr + (int64_t)bj * rows1;
    const uint32_t i_base = (uint32_t)bi * LOW_G_TILE, j_base = (uint32_t)bj * LOW_G_TILE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int WAVES = LOW_G_THREADS / 64;
    // (the words of a wave, as pair_low_kernel deals them; with ONE wave per workgroup -- ff_schedule.hpp LOW_G_THREADS
    // says why -- it is every word in turn)
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
        uint32_t a0 = 0, na = 0, b0 = 0, nbb = 0;
        float lr = 0.0f;
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
            if (r >= 0) {  // the row's lists in the two blocks, and its binary32 length: once per row
                a0 = pi[r];
                na = pi[r + 1] - a0;
                b0 = pj[r];
                nbb = pj[r + 1] - b0;
                lr = llow[r];
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
            LowGRound r;
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
            r.ra0 = __shfl(a0, L, 64), r.rna = __shfl(na, L, 64), r.l = __shfl(lr, L, 64);
            r.eb = entries[r.on ? at : 0u];
            return r;
        };
        LowGRound cur = fetch(0);
        for (uint32_t k0 = 0; k0 < totalb; k0 += 64) {
            LowGRound nxt = cur;
            if (k0 + 64 < totalb) nxt = fetch(k0 + 64);  // (uniform)
            if (cur.on)
                low_g_walk_row<KIND, DIAGONAL>(entries + cur.ra0, cur.rna, cur.l, cur.eb, (char *)acc + (cur.eb.off >> LOW_G_COL_SHIFT), e, am1);
            cur = nxt;
        }
        }  // (trip)
    }
    __syncthreads();
    // the tile's slots: row i = i_base + li holds columns j_base .. of slot i (i - 1) / 2 + j -- contiguous in j
    for (int q = threadIdx.x; q < LOW_G_TILE * LOW_G_TILE; q += LOW_G_THREADS) {
        const int li = q / LOW_G_TILE, lj = q % LOW_G_TILE;
        const int64_t i = (int64_t)i_base + li, j = (int64_t)j_base + lj;
        if (i < row_begin || i >= row_end || i >= n_samples || j >= i) continue;
        glow[i * (i - 1) / 2 - slot_begin + j] = acc[q];
    }
}
