// K4 of SURVEY.md 2.3: exact brute-force top-k of Q . Bank^T (inner product) or ||q-b||^2 (L2) --
// what the reference asks of faiss.GpuIndexFlatIP / GpuIndexFlatL2 (hbird/nn/search_faiss.py:43-46,
// 84-90) -- as ONE persistent gfx950 kernel: fp32 MFMA (v_mfma_f32_32x32x2_f32) contraction over
// LDS-staged fragment tiles with a fused per-query running top-k; the distance matrix is never
// written to HBM.  A second small kernel merges the per-workgroup partial lists.
//
// Work decomposition (host-built work list, see hb_build_schedule):
//   pair = (query tile of 256 rows, bank tile of 256 rows); a workgroup (512 threads = 8 waves,
//   2 per SIMD, one workgroup per CU) walks segments of consecutive bank tiles for one query tile
//   and keeps that query tile's k-best lists in LDS.  Wave w owns query columns [32w, 32w+32) and
//   all 256 bank rows of the tile: acc[8] x f32x16 = 128 accumulator VGPRs, C[m = bank row][n = query]
//   so a lane's 128 scores all belong to ONE query (lane & 31) and are compared against one
//   register-resident threshold.
//
// Numerics: every score is a single k-ascending fp32 fmaf chain started from the bank row's init
// value (0 for IP, -0.5*||b||^2 for L2, -inf for padding rows) -- bit-exact against
// oracle/hbird_oracle.c:orc_knn_chain_f32.  Ordering key: (score descending, row id ascending).
#include "hbird_internal.h"
#include "../../include/hbird_hip.h"
#include <algorithm>
#include <array>
#include <mutex>
#include <cstring>
#include <map>

#include "hbird_knn_dev.h"
#include "hbird_rerank_dev.h"

// One stage = one k8 fragment group of the pair tile: 32 MFMAs per wave, in two halves of 16 (bank row tiles
// 0-3 = "X", 4-7 = "Y").  Fragments of the next half are fetched from LDS while the current half is in the
// matrix pipe; HBM->LDS copies run three stages ahead (4-slot ring, hand-counted vmcnt).  Every non-MFMA
// instruction of the stage (9 ds_read_b128, 2 LDS-DMA copies, scalar bookkeeping) is pinned into its own gap
// between two MFMAs so that the 64-cycle matrix op ahead of it hides its issue.
#define KN_MFMA(T, FR, B, S) acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(FR[(T) & 3][S], B[S], acc[T], 0, 0, 0);

// COLD: the small-search instantiation -- cold start of a slot's first tile, scan epilogue, per-tile exchange of threshold floors
// (used for searches with few tiles per workgroup).
// CL: support for L2-sharing clusters (strided segments, soft sync).  A separate instantiation: its extra scalar state
// spilled SGPRs inside the stage loop of the pool (WIDE) instantiation (k = 90: +12 % kernel time).
// (The timing-only ablation instantiations of rounds 1-3 -- no copies / no fragment reads / no barrier / no epilogue -- and the
// in-kernel counters of the small-search work are gone from the product: their numbers are in profiles/LABBOOK.md and profiles/r01 - r03.)
// CEIL (pools only): a later pass of a search with k > 256 (hb_launch_knn_bigk) -- the tile's epilogue only queues rows strictly behind the
// query's ceiling key (the last neighbour already delivered): tile_epilogue<.., CEIL>
template <bool COLD, bool WIDE, bool CL = false, bool CEIL = false>
__global__ __launch_bounds__(HB_THREADS, 2) void knn_fused_kernel(knn_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    float* lst_s = reinterpret_cast<float*>(smem + KN_LISTS);
    unsigned* lst_i = reinterpret_cast<unsigned*>(smem + KN_LISTS + HB_QT * HB_KL * 4);
    float* sc = reinterpret_cast<float*>(smem + KN_SCRATCH) + w * 256;
    unsigned* qf = reinterpret_cast<unsigned*>(smem + KN_QF) + w * 512;   // small-search instantiation: landing zone of the quota floors
    int* pcnt = reinterpret_cast<int*>(smem + KN_LISTS);
    const int g8 = a.g8, k = a.k;   // g8 = stages per bank tile
    const int myq = w * 32 + (lane & 31);
    cl_sync cs;
    if constexpr (CL) cs = cl_init(a.wg_member, a.prog, a.cl, a.lag, blockIdx.x, w == 0, smem + KN_CLWORDS);

    wg_stamp<knn_args>(0);   // (every kNN kernel stamps: the share calibration reads whatever kernel the launcher picked)
    const int seg_begin = a.wg_off[blockIdx.x], seg_end = a.wg_end[blockIdx.x];   // this launch's share of the block's segments (phases: hb_launch_knn)
    // "everything before my first segment is done" (a member without any work: everything)
    if constexpr (CL) { if (w == 0) cl_publish(cs, seg_begin < seg_end ? a.segs[seg_begin].tile0 * g8 : 0x7FFFFFFF, lane); }
    for (int si = seg_begin; si < seg_end; ++si) {
        const hb_seg seg = a.segs[si];
        const int klw = a.klw;   // list row stride (HB_KL on the LDS path)
        const int bstride = CL ? seg.stride : 1, clock0 = CL ? seg.tile0 * g8 : 0;
        float* wl_s = a.state_s + (size_t)seg.slot * HB_QT * klw;      // this slot's lists in global memory
        unsigned* wl_i = a.state_i + (size_t)seg.slot * HB_QT * klw;
        float thr;
        if constexpr (WIDE) {
            // k > HB_KL: candidate pools in global memory, fill counts in the (otherwise unused) LDS list area
            thr = pool_begin(knn_args_pool_view{a.state_cnt, a.state_thr}, seg.slot, seg.first, pcnt, myq, lane);
        } else {
            // load (or start) this query tile's partial lists; each wave owns its 32 queries
            for (int e = lane; e < 1024; e += 64) {
                lst_s[w * 1024 + e] = seg.first ? -INFINITY : wl_s[w * 1024 + e];
                lst_i[w * 1024 + e] = seg.first ? HB_ID_NONE : wl_i[w * 1024 + e];
            }
            thr = lst_s[myq * HB_KL + (k - 1)];
        }
        thr = fmaxf(thr, floor_load(a.gthr, seg.q_tile * HB_QT + myq));
        const float* qsrc = a.q_tiles + ((size_t)(seg.q_tile * 8 + w) * g8) * HB_BLK + lane * 4;
        const int total = seg.n_tiles * g8;
        f32x16 acc[8];
        f32x4 fa[4], fy[4], fb, fbk;   // X-half / Y-half bank fragments, query fragment (current, kept for Y)

        int fpar = 0, cpar = 0;   // row-init double buffer: parity of the tile being fetched / computed
        // wave w stages bank row-tile w and query row-tile w of one k8 group (1 KiB each)
        // Only waves 0-3 issue the LDS-DMA copies (4 per stage each: bank row-tiles w, w+4 and query row-tiles
        // w, w+4).  Waves w and w+4 share a SIMD: when both stalled on a copy's issue at the same point of the
        // stage the matrix pipe idled; with one issuer per SIMD the partner keeps it fed (+3.1 % measured).
        auto issue_a = [&](int bt, int ks, int slot) {
            const float* src = a.bank_tiles + ((size_t)(bt * 8 + w) * g8 + ks) * HB_BLK + lane * 4;
            if (w < 4) {
                glds16(src, smem + slot * KN_SLOT_BYTES + w * 1024);
                glds16(src + (size_t)4 * g8 * HB_BLK, smem + slot * KN_SLOT_BYTES + (w + 4) * 1024);
            }
        };
        auto issue_b = [&](int bt, int ks, int slot) {
            const float* src = qsrc + (size_t)ks * HB_BLK;
            if (w < 4) {
                glds16(src, smem + slot * KN_SLOT_BYTES + 8192 + w * 1024);
                glds16(src + (size_t)4 * g8 * HB_BLK, smem + slot * KN_SLOT_BYTES + 8192 + (w + 4) * 1024);
            }
            if (ks == 0 && w == 0) glds16(a.binit + (size_t)bt * HB_BT + lane * 4, smem + KN_BINIT + (CL ? fpar : (bt & 1)) * 1024);
        };

        int bt = seg.b_tile0, ks = 0;          // stage being computed
        int fbt = seg.b_tile0, fks = 0;        // next stage to fetch
        int slot_c = 0, slot_f = 0;            // ring slots of the computed / fetched stage
        int left = total;                      // stages not yet fetched
        // After the last real stage the fetch position stays put and the (free) slot is re-filled with the same
        // stage: the steady-state loop has no data-dependent branches around its LDS traffic, so the compiler
        // counts its lgkmcnt waits instead of draining.
        auto advance_fetch = [&]() {
            if (--left > 0) { if (++fks == g8) { fks = 0; fbt += bstride; if constexpr (CL) fpar ^= 1; } }
            if (++slot_f == KN_RING) slot_f = 0;
        };
        // vmcnt is counted by hand (the compiler does not wait for LDS-DMA at a barrier): an issuing wave has
        // exactly four copies per stage in flight (wave 0 a fifth, the row-init values, at the first stage of a
        // tile), so "all but the newest 4" covers everything up to and including the stage about to be published.
        for (int p = 0; p < KN_RING - 1; ++p) { issue_a(fbt, fks, slot_f); issue_b(fbt, fks, slot_f); advance_fetch(); }
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // stage 0 landed; stages 1-2 in flight
        __syncthreads();
        {
            const f32x4* A = reinterpret_cast<const f32x4*>(smem);
#pragma unroll
            for (int t = 0; t < 4; ++t) fa[t] = A[t * 64 + lane];
            fb = reinterpret_cast<const f32x4*>(smem + 8192)[w * 64 + lane];
        }
        for (int st = 0; st < total; ++st) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // my copies of stage st+1 have landed (st+2 in flight)
            __syncthreads();   // ... everyone's have; the slot of stage st-1 is free for stage st+3
            int slot_n = slot_c + 1; if (slot_n == KN_RING) slot_n = 0;
            const f32x4* Ac = reinterpret_cast<const f32x4*>(smem + slot_c * KN_SLOT_BYTES) + lane;
            const f32x4* An = reinterpret_cast<const f32x4*>(smem + slot_n * KN_SLOT_BYTES) + lane;
            // small searches: the floors of this tile come in by LDS-DMA during its last four stages (older than the stage's copies:
            // the hand-counted vmcnt still holds; four stages of counted waits cover them) and are read at its end -- requested at
            // the tile's START they were one tile staler: 50,176 x 384 4.62 -> 4.53 ms on the kernel with register-resident fragments
            if constexpr (COLD && !WIDE) { if (ks == (g8 > 4 ? g8 - 4 : 0)) small_floor_request(a.qfl, a.gthr, seg, w, lane, qf, sc); }
            if (ks == 0) {
                const f32x4* bi = reinterpret_cast<const f32x4*>(smem + KN_BINIT + (CL ? cpar : (bt & 1)) * 1024);
#pragma unroll
                for (int t = 0; t < 8; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v = bi[8 * t + 2 * g + h];
                        acc[t][4 * g + 0] = v[0]; acc[t][4 * g + 1] = v[1];
                        acc[t][4 * g + 2] = v[2]; acc[t][4 * g + 3] = v[3];
                    }
            }
            // ---- X half: tiles 0-3, k-steps 0-3; fillers: the four Y fragments, the two LDS-DMA copies ----
            KN_FENCE KN_MFMA(0, fa, fb, 0) KN_FENCE fy[0] = Ac[4 * 64];
            KN_FENCE KN_MFMA(1, fa, fb, 0) KN_FENCE fy[1] = Ac[5 * 64];
            KN_FENCE KN_MFMA(2, fa, fb, 0) KN_FENCE fy[2] = Ac[6 * 64];
            KN_FENCE KN_MFMA(3, fa, fb, 0) KN_FENCE fy[3] = Ac[7 * 64];
            KN_FENCE KN_MFMA(0, fa, fb, 1) KN_MFMA(1, fa, fb, 1) KN_FENCE
            // cluster soft sync: wave 0 pays the issue of one more vector-memory instruction now and then (its SIMD partner
            // covers it like it covers the copies); issued AHEAD of the stage's copies, so the hand-counted vmcnt still holds
            if constexpr (CL) { if (w == 0) cl_tick(cs, clock0 + st, lane); }
            issue_a(fbt, fks, slot_f);
            KN_FENCE KN_MFMA(2, fa, fb, 1) KN_MFMA(3, fa, fb, 1) KN_MFMA(0, fa, fb, 2) KN_MFMA(1, fa, fb, 2) KN_FENCE
            issue_b(fbt, fks, slot_f);
            KN_FENCE KN_MFMA(2, fa, fb, 2) KN_MFMA(3, fa, fb, 2) KN_FENCE
            advance_fetch();
            KN_FENCE KN_MFMA(0, fa, fb, 3) KN_MFMA(1, fa, fb, 3) KN_MFMA(2, fa, fb, 3) KN_MFMA(3, fa, fb, 3) KN_FENCE
            fbk = fb;   // the Y half still needs this stage's query fragment
            // ---- Y half: tiles 4-7; fillers: the X fragments and the query fragment of stage st+1 ----
            KN_FENCE KN_MFMA(4, fy, fbk, 0) KN_FENCE fa[0] = An[0 * 64];
            KN_FENCE KN_MFMA(5, fy, fbk, 0) KN_FENCE fa[1] = An[1 * 64];
            KN_FENCE KN_MFMA(6, fy, fbk, 0) KN_FENCE fa[2] = An[2 * 64];
            KN_FENCE KN_MFMA(7, fy, fbk, 0) KN_FENCE fa[3] = An[3 * 64];
            KN_FENCE KN_MFMA(4, fy, fbk, 1) KN_FENCE
            fb = reinterpret_cast<const f32x4*>(smem + slot_n * KN_SLOT_BYTES + 8192)[w * 64 + lane];
            KN_FENCE
            KN_MFMA(5, fy, fbk, 1) KN_MFMA(6, fy, fbk, 1) KN_MFMA(7, fy, fbk, 1)
            KN_MFMA(4, fy, fbk, 2) KN_MFMA(5, fy, fbk, 2) KN_MFMA(6, fy, fbk, 2) KN_MFMA(7, fy, fbk, 2)
            KN_MFMA(4, fy, fbk, 3) KN_MFMA(5, fy, fbk, 3) KN_MFMA(6, fy, fbk, 3) KN_MFMA(7, fy, fbk, 3)
            KN_FENCE
            slot_c = slot_n;
            if (++ks == g8) {
                if constexpr (WIDE) {
                    // the slot's pool pointers are derived HERE (from one scalar, laundered so that the compiler cannot
                    // hoist them): kept live through the stage loop they crowd out the copy loop's own pointers, which
                    // then come back from spilled SGPRs in every stage (k = 90: +10 % kernel time)
                    int slot_ = seg.slot;
                    asm volatile("" : "+s"(slot_));
                    float* ps = a.state_s + (size_t)slot_ * HB_QT * klw;
                    unsigned* pi = a.state_i + (size_t)slot_ * HB_QT * klw;
                    if constexpr (CEIL) {
                        // (the ceiling is read HERE, once per tile, not kept in registers through the stage loop)
                        const float c_s = a.ceil_s[seg.q_tile * HB_QT + myq];
                        const unsigned c_i = a.ceil_i[seg.q_tile * HB_QT + myq];
                        tile_epilogue<true, true, HB_POOL_MAX / 64, true>(acc, thr, ps, pi, sc, w * 32, lane, k, (unsigned)bt, klw, pcnt, c_s, c_i);
                    } else tile_epilogue<true, true>(acc, thr, ps, pi, sc, w * 32, lane, k, (unsigned)bt, klw, pcnt);
                } else if constexpr (COLD) {
                    // small searches: cold start of a slot's first tile (separate instantiation, see launcher)
                    if (seg.first && bt == seg.b_tile0 && cold_start_needed(thr)) thr = fmaxf(thr, cold_start_threshold(acc, k));
                    // the floors requested four stages ago (waves 4-7 have nothing else in flight; waves 0-3 have passed
                    // counted waits that cover them -- except in a one-stage tile, D <= 8)
                    if (g8 < 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    asm volatile("s_cmp_lt_u32 %0, 4\n\ts_cbranch_scc1 .Lfl_%=\n\ts_waitcnt vmcnt(0)\n.Lfl_%=:" :: "s"(w) : "memory", "scc");
                    thr = fmaxf(thr, small_floor_read(seg, qf, sc, lane));
                    // (few rows per slot -> many insertions per tile): scan + register queue; the big searches keep the plain
                    // epilogue (insertions are rare there, and the scan's registers would spill)
                    list_epilogue_scan(acc, thr, lst_s, lst_i, w * 32, lane, k, (unsigned)bt);
                    small_floor_publish(a.qfl, a.gthr, seg, lst_s, myq, k, thr, lane);
                } else tile_epilogue<true, false>(acc, thr, lst_s, lst_i, sc, w * 32, lane, k, (unsigned)bt);
                ks = 0;
                bt += bstride; if constexpr (CL) cpar ^= 1;
            }
        }
        if constexpr (CL) { if (w == 0) cl_publish(cs, seg.next_tile0 == 0x7FFFFFFF ? 0x7FFFFFFF : seg.next_tile0 * g8, lane); }   // covers idle units
        if constexpr (!WIDE) {   // store the partial lists of this segment
            for (int e = lane; e < 1024; e += 64) { wl_s[w * 1024 + e] = lst_s[w * 1024 + e]; wl_i[w * 1024 + e] = lst_i[w * 1024 + e]; }
        } else {
            pool_end(knn_args_pool_view{a.state_cnt, a.state_thr}, seg.slot, pcnt, thr, myq, lane);
        }
        if (lane < 32) floor_publish(a.gthr, seg.q_tile * HB_QT + myq, thr);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the (unused) run-ahead copies
        __syncthreads();   // the ring is reused by the next segment's prologue
    }
    if constexpr (CL) cl_finish(cs, a.cl_stats, w == 0, lane);
    wg_stamp<knn_args>(1);
}

// ---- merge of the partial lists of one query: rank by counting over <= slots*k candidates --------
// Slot selection of a merge block: either the work list's slots of the query tile (qt_slots) or, in the second
// level of a two-level merge, the `fixed_ng` group lists written by the first level (slot = qt * fixed_ng + j).
// grp_size > 0 (first level): block (q, grp) merges only slots [grp*grp_size, (grp+1)*grp_size) of its query tile
// and writes a sorted list of k entries (row stride klw) into (tmp_s, tmp_i) slot qt * n_groups + grp.
// A slot holds `per` entries per query: a sorted list (per = k, sentinel-padded) or, with cnts != nullptr, an
// unsorted candidate pool of which the first cnts[slot][query] entries are valid.
__global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ state_s,
                                                       const unsigned* __restrict__ state_i,
                                                       const int* __restrict__ cnts, const float* __restrict__ pthr, int per,
                                                       const int* __restrict__ qt_off, const int* __restrict__ qt_slots,
                                                       int fixed_ng, int grp_size, int n_groups, float* __restrict__ tmp_s,
                                                       unsigned* __restrict__ tmp_i,
                                                       int64_t nq, int k, int klw, int64_t id_base, int metric,
                                                       const float* __restrict__ qn2, int64_t* __restrict__ out_idx,
                                                       float* __restrict__ out_dist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t q = blockIdx.x;
    const int grp = blockIdx.y;
    const int qt = (int)(q / HB_QT), ql = (int)(q % HB_QT);
    int s0, ns;
    if (fixed_ng > 0) { s0 = qt * fixed_ng; ns = fixed_ng; }
    else { s0 = qt_off[qt]; ns = qt_off[qt + 1] - s0; }
    if (grp_size > 0) {
        const int lo = min(ns, grp * grp_size), hi = min(ns, lo + grp_size);
        s0 += lo; ns = hi - lo;
    }
    float* cs = reinterpret_cast<float*>(smem);
    unsigned* ci = reinterpret_cast<unsigned*>(smem) + ns * per;
    const int lane = threadIdx.x;
    // Pre-filter: a slot that knows k candidates reaching v (a sorted list: its k-th entry; a pool: the threshold of its last
    // compaction, or a foreign floor it ran under -- both lower bounds of the k-th best of the union) rules out everything
    // below the largest such v.  With many slots per query tile (few queries against a big bank: one slot per workgroup) the
    // rank-by-counting below is quadratic in slots x k: 1,369 queries x 200 k rows in use_fp16 mode spent 20 ms here.
    float tstar = -INFINITY;
    for (int j = lane; j < ns; j += 64) {
        const int sl = fixed_ng > 0 ? s0 + j : qt_slots[s0 + j];
        const size_t oq = (size_t)sl * HB_QT + ql;
        if (cnts) { if (pthr && cnts[oq] >= k) tstar = fmaxf(tstar, pthr[oq]); }
        else tstar = fmaxf(tstar, state_s[oq * klw + (k - 1)]);
    }
    for (int o = 32; o > 0; o >>= 1) tstar = fmaxf(tstar, __shfl_xor(tstar, o));
    // gather the surviving candidates of the slots, densely packed
    int n = 0;
    for (int j = 0; j < ns; ++j) {
        const int sl = fixed_ng > 0 ? s0 + j : qt_slots[s0 + j];
        const int valid = cnts ? min(per, cnts[(size_t)sl * HB_QT + ql]) : per;
        const size_t off = ((size_t)sl * HB_QT + ql) * klw;
        // all of a slot's entries (at most HB_POOL_MAX = 8 x 64) are requested before the first is looked at: the loop used to wait for a
        // score, then for its id, 64 entries at a time -- two memory round trips per 64 entries, 1.18 of a 15.6 ms search at k = 90
        float vv[HB_POOL_MAX / 64];
        unsigned vi[HB_POOL_MAX / 64];
#pragma unroll
        for (int u = 0; u < HB_POOL_MAX / 64; ++u) {
            const int e = u * 64 + lane;
            vv[u] = -INFINITY; vi[u] = 0u;
            if (e < valid) { vv[u] = state_s[off + e]; vi[u] = state_i[off + e]; }
        }
#pragma unroll
        for (int u = 0; u < HB_POOL_MAX / 64; ++u) {
            if (u * 64 >= valid) break;
            const int e = u * 64 + lane;
            // (sentinel entries -- the padding of a sorted list with fewer than k rows -- stay behind: a seeded second pass of few queries
            // leaves 22 group lists of 256 entries with a hundred real candidates among them, and the ranking below is quadratic: 18 ms
            // for two queries, profiles/r06/fp16_escalation_merge_before.csv)
            const bool keep = e < valid && vi[u] != HB_ID_NONE && (vv[u] >= tstar || tstar == -INFINITY);
            const unsigned long long m = __ballot(keep);
            if (keep) { const int pos = n + __popcll(m & ((1ull << lane) - 1ull)); cs[pos] = vv[u]; ci[pos] = vi[u]; }
            n += __popcll(m);
        }
    }
    // Still many: keep about k of them, so that the rank-by-counting below sees about k candidates instead of slots x k (it is quadratic:
    // 6,144 candidates of 32 pools took a wave 0.4 ms).  A bisection over the monotone keys finds a cut with k .. k + 32 candidates above
    // it (one pass over the candidates per round, counted 64 at a time by ballot; it stops as soon as the count fits: about eight rounds;
    // until round 4 a radix select of the exact k-th key ran here, always 32 rounds: 1.18 of a 15.6 ms use_fp16 search at 300,000 x 768,
    // k = 90) -- every candidate that can rank below k lies above the cut, ties of the k-th included.  Scores that the bisection cannot
    // separate (24 rounds) go through the radix select.
    if (n > k + 64) {                // (the ranking below is quadratic: from k + 64 candidates on a cut pays)
        unsigned cut = 0;            // keep keys > cut
        {
            unsigned lo = 0, hi = 0xFFFFFFFFu;     // at least k keys above lo (all n: no score has key 0), fewer than k above hi
            int clo = n;
            for (int r = 0; r < 24 && hi - lo > 1u && clo > k + 32; ++r) {
                const unsigned mid = lo + ((hi - lo) >> 1);
                int c = 0;
                for (int base = 0; base < n; base += 64) {
                    const int idx = base + lane;
                    c += __popcll(__ballot(idx < n && pool_key(cs[idx]) > mid));
                }
                if (c >= k) { lo = mid; clo = c; } else hi = mid;
            }
            cut = lo;
            if (clo > k + 64 && clo > 2 * k) {   // not separated: the exact k-th key (its ties stay)
                unsigned prefix = 0;
                int kk = k;
                for (int b = 31; b >= 0; --b) {
                    const unsigned himask = ~((1u << b) - 1u), want = prefix | (1u << b);
                    int c = 0;
                    for (int base = 0; base < n; base += 64) {
                        const int idx = base + lane;
                        c += __popcll(__ballot(idx < n && (pool_key(cs[idx]) & himask) == want));
                    }
                    if (c >= kk) prefix = want; else kk -= c;
                }
                cut = prefix - 1u;    // (prefix >= 1: the key of a score)
            }
        }
        int m = 0;
        for (int base = 0; base < n; base += 64) {   // in place: a kept entry moves to a position at or below its own
            const int idx = base + lane;
            const float v = idx < n ? cs[idx] : 0.0f;
            const unsigned id = idx < n ? ci[idx] : 0u;
            const bool keep = idx < n && pool_key(v) > cut;
            const unsigned long long mk = __ballot(keep);
            if (keep) { const int pos = m + __popcll(mk & ((1ull << lane) - 1ull)); cs[pos] = v; ci[pos] = id; }
            m += __popcll(mk);
        }
        n = m;
    }
    const size_t tmp_off = grp_size > 0 ? ((size_t)(qt * n_groups + grp) * HB_QT + ql) * klw : 0;
    __syncthreads();
    for (int c = lane; c < n; c += 64) {
        const float s = cs[c];
        const unsigned id = ci[c];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = cs[j];
            const unsigned ij = ci[j];
            rank += (sj > s) || (sj == s && (ij < id || (ij == id && j < c)));
        }
        if (rank < k) {
            if (grp_size > 0) { tmp_s[tmp_off + rank] = s; tmp_i[tmp_off + rank] = id; continue; }
            const int64_t o = q * (int64_t)k + rank;
            if (id == HB_ID_NONE) {
                out_idx[o] = -1;
                out_dist[o] = metric == 1 ? INFINITY : -INFINITY;
            } else {
                out_idx[o] = (int64_t)id + id_base;
                if (metric == 1) { const float d2 = fmaf(-2.0f, s, qn2[q]); out_dist[o] = d2 > 0.0f ? d2 : 0.0f; }
                else out_dist[o] = s;
            }
        }
    }
    for (int r = n + lane; r < k; r += 64) {   // fewer than k candidates: missing neighbours
        if (grp_size > 0) { tmp_s[tmp_off + r] = -INFINITY; tmp_i[tmp_off + r] = HB_ID_NONE; continue; }
        out_idx[q * (int64_t)k + r] = -1;
        out_dist[q * (int64_t)k + r] = metric == 1 ? INFINITY : -INFINITY;
    }
}

// Merge the partial lists / pools of every query: one level when the candidates of a query tile's slots fit the merge
// block's LDS, two levels otherwise (few query tiles against a big bank: up to one slot per workgroup).
// cnts == nullptr: sorted lists of k entries; otherwise pools of capacity klw with fill counts cnts.
static int launch_merge(hb_index* ix, const float* state_s, const unsigned* state_i, const int* cnts, const float* pthr, const int* qt_off,
                        const int* qt_slots, int max_slots, int nqt, int64_t nq, int k, int klw, int64_t id_base, int metric,
                        const float* qn2, int64_t* out_idx, float* out_dist, hipStream_t s) {
    const size_t lim = 48 * 1024;
    const int per = cnts ? klw : k;
    if ((size_t)max_slots * per * 8 <= lim) {
        knn_merge_kernel<<<dim3((unsigned)nq), dim3(64), (size_t)max_slots * per * 8, s>>>(state_s, state_i, cnts, pthr, per, qt_off, qt_slots,
                                                                                            0, 0, 0, nullptr, nullptr, nq, k, klw,
                                                                                            id_base, metric, qn2, out_idx, out_dist);
        HB_HIP(hipGetLastError());
        return 0;
    }
    const int grp = std::max<int>(2, (int)(lim / ((size_t)per * 8)));
    const int ng = (max_slots + grp - 1) / grp;
    if ((size_t)ng * k * 8 > lim) return hb_fail("hb_index_search: too many partial lists per query tile for the merge kernel");
    const size_t half = (size_t)nqt * ng * HB_QT * klw * 4;
    if (ix->mtmp.ensure(2 * half, HB_GROW_QUARTER)) return -1;
    float* ts = ix->mtmp.as<float>();
    unsigned* ti = ix->mtmp.as<unsigned>(half);
    knn_merge_kernel<<<dim3((unsigned)nq, (unsigned)ng), dim3(64), (size_t)grp * per * 8, s>>>(state_s, state_i, cnts, pthr, per, qt_off, qt_slots,
                                                                                                0, grp, ng, ts, ti, nq, k, klw, 0, 0,
                                                                                                nullptr, nullptr, nullptr);
    HB_HIP(hipGetLastError());
    knn_merge_kernel<<<dim3((unsigned)nq), dim3(64), (size_t)ng * k * 8, s>>>(ts, ti, nullptr, nullptr, k, nullptr, nullptr, ng, 0, 0, nullptr,
                                                                                nullptr, nq, k, klw, id_base, metric, qn2, out_idx,
                                                                                out_dist);
    HB_HIP(hipGetLastError());
    return 0;
}

// ---- merge of per-shard results [parts][nq][k] (multi-GPU: after the all-gather) -------------------
// IP: larger is better; L2: smaller squared distance is better.  Ties -> lower global id.
// A part's lists start at dist_parts + p * dist_stride / idx_parts + p * idx_stride (elements): [parts][nq][k] arrays
// (stride nq*k) or the packed per-rank buffers of one all-gather (hb_merge_topk_packed).
__global__ __launch_bounds__(64) void merge_parts_kernel(const float* __restrict__ dist_parts,
                                                         const int64_t* __restrict__ idx_parts, int parts, int64_t nq,
                                                         int k, int metric, int64_t dist_stride, int64_t idx_stride,
                                                         int64_t* __restrict__ out_idx, float* __restrict__ out_dist) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t q = blockIdx.x;
    const int n = parts * k;
    float* cs = reinterpret_cast<float*>(smem);
    int64_t* ci = reinterpret_cast<int64_t*>(smem + ((n * 4 + 15) / 16) * 16);
    const int lane = threadIdx.x;
    for (int c = lane; c < n; c += 64) {
        const size_t off = (size_t)q * k + (c % k);
        float d = dist_parts[(size_t)(c / k) * dist_stride + off];
        cs[c] = metric == 1 ? -d : d;
        ci[c] = idx_parts[(size_t)(c / k) * idx_stride + off];
    }
    __syncthreads();
    for (int c = lane; c < n; c += 64) {
        const float s = cs[c];
        const int64_t id = ci[c];
        // missing neighbours (id < 0) sort last
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = cs[j];
            const int64_t ij = ci[j];
            bool better;
            if (ij < 0 || id < 0) better = (ij >= 0 && id < 0) || (ij < 0 && id < 0 && j < c);
            else better = (sj > s) || (sj == s && (ij < id || (ij == id && j < c)));
            rank += better;
        }
        if (rank < k) {
            const int64_t o = q * (int64_t)k + rank;
            out_idx[o] = id < 0 ? -1 : id;
            out_dist[o] = id < 0 ? (metric == 1 ? INFINITY : -INFINITY) : (metric == 1 ? -s : s);
        }
    }
}

int hb_launch_merge_parts(const float* dist_parts, const int64_t* idx_parts, int parts, int64_t nq, int k, int metric,
                          int64_t dist_stride, int64_t idx_stride, int64_t* out_idx, float* out_dist, hipStream_t s) {
    if (nq == 0) return 0;
    const size_t n = (size_t)parts * k;
    const size_t sh = ((n * 4 + 15) / 16) * 16 + n * 8;
    if (sh > 60000) return hb_fail("hb_merge_topk: parts*k too large for the merge kernel");
    merge_parts_kernel<<<dim3((unsigned)nq), dim3(64), sh, s>>>(dist_parts, idx_parts, parts, nq, k, metric, dist_stride, idx_stride,
                                                                 out_idx, out_dist);
    HB_HIP(hipGetLastError());
    return 0;
}

// (the host-side work list -- hb_build_schedule and friends -- lives in hbird_schedule.cpp: plain C++, also built host-only under sanitizers)

// Phased searches (pools: k > HB_KL and the fp16 candidate pass).  A pool's threshold is the k-th best of ONE slot's share of the rows
// and only rises when the pool is compacted: with S slots per query tile every slot re-discovers what the others already know, and
// what the pools' epilogue costs is the candidates it appends, not the test (measured with perfect floors -- a repeated search that
// starts from the previous one's final floors: fp16 candidate kernel 29.2 -> 19.4 ms at 2,074,072 x 384, 317 -> 300 ms at 10 M x 768;
// 18.1 ms without any epilogue).  So the search is launched in PHASES of growing size -- every workgroup's segment list cut at the
// same clocks (hb_build_schedule; whole segments per phase left most workgroups idle in the small phases and was slower than no
// phases at all) -- and between two phases the slots' pools are merged (the merge kernel of the final result) and the k-th best of
// ALL rows seen so far becomes every slot's floor: exactly the union's k-th best, so the results keep their bits.  Same box, kernel
// ms without / with phases: fp16 k = 30: 50,176 x 384 4.62 / 2.30, 300 k x 768 12.35 / 8.45, 1 M x 1024 (4,096 queries) 12.9 /
// 8.95, 2,074,072 x 384 29.6 / 25.3, 10 M x 768 321.6 / 317; fp32: k = 90 50,176 x 384 9.75 / 6.2, k = 64 300 k x 768 51.2 / 44.8,
// k = 90 2,074,072 x 384 161.4 / 146.1.  The LDS lists (k <= 32) stay unphased: their slots already exchange floors every tile
// (small_floor_*) and phases only added launches (50,176 x 384: 4.72 -> 4.86-5.19 ms).
__global__ __launch_bounds__(256) void seed_floors_kernel(const int64_t* __restrict__ idx, const float* __restrict__ score, int64_t nq, int kk,
                                                         unsigned* __restrict__ gthr) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    if (idx[q * kk + kk - 1] >= 0) atomicMax(gthr + q, pool_key(score[q * kk + kk - 1]));   // kk rows reach this score: a floor (ties pass)
}

__global__ __launch_bounds__(256) void seed_from_scores_kernel(const float* __restrict__ seed, int64_t nq, unsigned* __restrict__ gthr) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const float v = seed[q];
    if (v > -INFINITY && v < INFINITY) atomicMax(gthr + q, pool_key(v));      // rows scoring >= v pass (floor_from_key admits ties); NaN / inf: no seed
}

// The same floor straight from the pools, without the merge: one wave per query gathers the scores of its slots' pools (those that
// can matter: at or above the best threshold a full pool already has) into LDS and bisects for a score that at least kk of them
// exceed -- 14 halvings between the smallest and the largest; any such score is a valid floor (cold_start_threshold,
// hbird_knn_dev.h).  The merge kernel ranks its candidates by counting (quadratic) and writes int64 ids: 85-150 us per phase
// boundary for 12,544 queries against 25-30 here.
__global__ __launch_bounds__(256) void pool_floor_kernel(const float* __restrict__ state_s, const int* __restrict__ cnts,
                                                        const float* __restrict__ pthr, const int* __restrict__ qt_off,
                                                        const int* __restrict__ qt_slots, int64_t nq, int kk, int klw, int per_wave,
                                                        unsigned* __restrict__ gthr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // (one query per wave: a launch of its own has all the parallelism it wants -- a two-queries-per-wave form, one per lane half, built in round 5
    // for floors computed inside the kNN kernels, measured 25 us per boundary SLOWER here)
    const int64_t q = (int64_t)blockIdx.x * 4 + w;
    if (q >= nq) return;
    pool_floor_query(state_s, cnts, pthr, qt_off, qt_slots, q, kk, klw, reinterpret_cast<float*>(smem) + (size_t)w * per_wave, gthr, lane);
}

// Per-XCD work shares, calibrated.  The eight XCDs of an MI355X do not run the fp32 kernel at one speed: with equal work the workgroups of
// the odd XCDs finish 1-2 % after those of the even ones (profiles/r05/xcd_speed_stamps_headline.txt), and a launch lasts as long as its
// slowest workgroup.  Big fp32 searches therefore stamp every workgroup's start and end (two stores per block), the stamps travel to pinned
// host memory behind the launch, and the NEXT such search -- if that copy has completed; it never waits for it -- turns each XCD group's
// median duration into its share of the work list: share_x <- share_x x (median of all / median of group x).  One round brings the groups
// within 0.1-0.3 % of each other (10 M x 768: 2275 -> 2258 ms, 2.5 M x 768: 573.7 -> 568.4; profiles/r05/xcd_weights_iterated.txt); later
// rounds only act on a change beyond 0.3 %.  Speed only: any shares give the same results.  The fp16 candidate kernel calibrates shares of its own (its
// XCDs differ by other amounts: it runs on the chip's power budget): 274.0 -> 270.0 ms at 10 M x 768, 18.6 -> 18.4 at 2 M x 384 -- but only
// since a phased list's cuts follow the shares (hb_finish_schedule); with common cuts, where a group's extra share lands in the last phase,
// the same shares made it SLOWER (281 -> 288-297 ms).  Shares are remembered per device and family for indexes created later.
static std::mutex g_xcd_mu;
static std::map<std::pair<int, int>, std::array<double, 8>> g_xcd_known;     // (device, kernel family) -> last calibrated shares
static std::map<int, int> g_cl_known;                                        // device -> decided: fp32 clusters on (1) / off (0)
static void hb_xcd_calibrate(hb_index* ix, int fam) {
    hb_index::xcd_cal& c = ix->xcal[fam];
    if (c.rounds == 0 && !c.stamp_pending) {        // a new index starts from what this device is known to need
        std::lock_guard<std::mutex> lock(g_xcd_mu);
        auto it = g_xcd_known.find({ix->device, fam});
        if (it != g_xcd_known.end()) {
            bool differs = false;
            for (int x = 0; x < 8; ++x) { differs = differs || c.w[x] != it->second[x]; c.w[x] = it->second[x]; }
            if (differs) ix->sched = hb_schedule();
            c.rounds = 1;
        }
        auto cl = g_cl_known.find(ix->device);
        if (fam == 0 && cl != g_cl_known.end() && c.cl_state != 2) { c.cl_state = 2; c.cl_choice = cl->second; ix->sched = hb_schedule(); }
    }
    if (!c.stamp_pending || !c.stamp_ev || !c.stamp_host || hipEventQuery(c.stamp_ev) != hipSuccess) { (void)hipGetLastError(); return; }
    const int G = c.stamp_pending;
    c.stamp_pending = 0;
    // the decisions themselves are plain host code (hbird_calibrate.cpp: also fed with synthetic stamps by tests/test_calibrate_cpu.py)
    hb_stamp_set set;
    set.stamps = c.stamp_host; set.G = G; set.key = c.stamp_key; set.frac = c.stamp_frac; set.auto_cluster = c.stamp_auto_cluster;
    for (int x = 0; x < 8; ++x) set.run_shares[x] = c.stamp_w[x];
    const int flags = hb_xcd_step(c, fam, set);
    if (flags & HB_CAL_REBUILD) ix->sched = hb_schedule();                     // rebuilt with the new shares / cluster form by the caller
    if (flags & (HB_CAL_REMEMBER_SHARES | HB_CAL_REMEMBER_CLUSTERS)) {
        std::lock_guard<std::mutex> lock(g_xcd_mu);
        if (flags & HB_CAL_REMEMBER_SHARES) {
            std::array<double, 8> keep;
            for (int x = 0; x < 8; ++x) keep[x] = c.w[x];
            g_xcd_known[{ix->device, fam}] = keep;
        }
        if (flags & HB_CAL_REMEMBER_CLUSTERS) g_cl_known[ix->device] = c.cl_choice;
    }
}
// behind a calibrating launch: its per-block stamps -> pinned host memory, read by the next big search of the family if the copy has completed by then
static int hb_xcd_collect(hb_index* ix, int fam, const unsigned* stamps_dev, const hb_schedule& sc, const double* shares, int n_phases, int nqt, int nbt,
                          int k, hipStream_t s, bool auto_cluster = false) {
    hb_index::xcd_cal& c = ix->xcal[fam];
    if (!stamps_dev || sc.G > 1024 || c.stamp_pending) return 0;
    if (!c.stamp_ev) HB_HIP(hipEventCreateWithFlags(&c.stamp_ev, hipEventDisableTiming));
    if (!c.stamp_host) HB_HIP(hipHostMalloc((void**)&c.stamp_host, 1024 * 32, hipHostMallocDefault));
    HB_HIP(hipMemcpyAsync(c.stamp_host, stamps_dev, (size_t)sc.G * 32, hipMemcpyDeviceToHost, s));
    HB_HIP(hipEventRecord(c.stamp_ev, s));
    c.stamp_pending = sc.G;
    for (int x = 0; x < 8; ++x) c.stamp_w[x] = shares[x];
    c.stamp_key = {nqt, nbt, sc.G, n_phases, k, sc.cq * 16 + sc.cb};
    c.stamp_auto_cluster = auto_cluster ? 1 : 0;
    // a phased search stamps its last launch.  Cuts that follow the shares (long lists, hb_finish_schedule) make it a fair sample; with
    // common cuts a group's extra share is all in that launch -- its part of the work
    const double per_wg = (double)nqt * (double)nbt / std::max(1, sc.G);
    c.stamp_frac = n_phases > 1 && !sc.cuts_scaled && per_wg > 0.0 ? std::min(1.0, std::max(0.25, 1.0 - (double)sc.phase_clock.back() / per_wg)) : 1.0;
    return 0;
}

// ---- k beyond the pools' 256 (the reference forwards any k to Faiss, search_faiss.py:84-85; faiss-gpu takes up to 2048) ------------------------
// The best k = the best 256, then the best 256 of the rows BEHIND those in the ordering (score descending, id ascending), and so on: passes of
// the pool search, each with a per-query ceiling key = the last neighbour delivered so far.  A pass costs a whole search (k = 1024: four), which
// is what an exact flat search of that width costs here; ids and distance bits are those of one search with a list of k.
__global__ __launch_bounds__(256) void bigk_place_kernel(const int64_t* __restrict__ tmp_idx, const float* __restrict__ tmp_sc, int64_t nq, int kp, int k,
                                                         int col0, int64_t id_base, int out_metric, const float* __restrict__ qn2,
                                                         int64_t* __restrict__ out_idx, float* __restrict__ out_dist, float* __restrict__ ceil_s,
                                                         unsigned* __restrict__ ceil_i) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq * kp) return;
    const int64_t q = t / kp;
    const int j = (int)(t % kp);
    const int64_t id = tmp_idx[t];
    const float s = tmp_sc[t];
    const int64_t o = q * (int64_t)k + col0 + j;
    if (id < 0) { out_idx[o] = -1; out_dist[o] = out_metric == 1 ? INFINITY : -INFINITY; }
    else {
        out_idx[o] = id + id_base;
        if (out_metric == 1) { const float d2 = fmaf(-2.0f, s, qn2[q]); out_dist[o] = d2 > 0.0f ? d2 : 0.0f; }
        else out_dist[o] = s;
    }
    if (j == kp - 1) {      // the next pass starts behind this entry; a list that ran out of rows closes the search (nothing is behind -inf)
        ceil_s[q] = id < 0 ? -INFINITY : s;
        ceil_i[q] = id < 0 ? 0xFFFFFFFFu : (unsigned)id;
    }
}

// What distinguishes ONE invocation of the launcher from the index's settings.  hb_launch_knn builds the level-0 call from the index; the
// passes of a search with k > 256 (hb_launch_knn_bigk) and the re-search of uncertified queries (knn_research_failures) build a new one for
// their nested search.  Nothing here is written to the index, so a nested search that fails leaves no trace in it.
struct knn_call {
    int esc = 0;                       // 0: a caller's search; 1: the second fp16 pass over its uncertified queries; 2: the fp32 search of what is left
    const float* seed = nullptr;       // per-query floors (scores) a nested search starts from
    const float* ceil_s = nullptr;     // a later pass of a search with k > 256: per query the ordering key of the last neighbour delivered
    const unsigned* ceil_i = nullptr;
    int fp16 = 0;                      // the fp16 setting in force for this call (hb_index::fp16 for a caller's search)
    bool timed = false;                // events around the kernel launches, workgroup stamps, last_knn_ms
    const float* q_aux = nullptr;      // [nq] chain ||q||^2 and [nq] fp32 norms of THIS call's queries
    bool score_out = false;            // the ordering score goes out as it is, whatever the metric
    // an excluding search on the screen (hb_launch_knn_excluding): per query the row group its re-rank drops among the candidates (nullptr: a
    // plain search) and (second pass) the caller's query number of each of this call's queries
    const int32_t* groups = nullptr;
    const int64_t* excl_orig = nullptr;
    // where the search reports and whose adaptive fp16 policy it follows and feeds: the caller-level entry's own (which it commits), or a
    // detached pair that nobody commits.  Nested calls get the same pointers and write their level's part in sequence.
    hb_search_report* rep = nullptr;
    hb_f16_adapt* adapt = nullptr;
};
static int knn_search(hb_index* ix, const knn_call& c, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist);

static int hb_launch_knn_bigk(hb_index* ix, const knn_call& c, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist) {
    if (nq == 0) return 0;
    hipStream_t s = ix->stream;
    const int64_t nqp = (nq + HB_QT - 1) / HB_QT * HB_QT;
    const size_t o_sc = al256((size_t)nq * 256 * 8), o_cs = o_sc + al256((size_t)nq * 256 * 4), o_ci = o_cs + al256((size_t)nqp * 4), tot = o_ci + al256((size_t)nqp * 4);
    if (ix->bigk.ensure(tot, HB_GROW_QUARTER)) return -1;
    int64_t* tmp_idx = ix->bigk.as<int64_t>();
    float* tmp_sc = ix->bigk.as<float>(o_sc);
    float* ceil_s = ix->bigk.as<float>(o_cs);
    unsigned* ceil_i = ix->bigk.as<unsigned>(o_ci);
    HB_HIP(hipMemsetD32Async((hipDeviceptr_t)ceil_s, 0xFF800000u, (size_t)nqp, s));      // (padding queries: nothing behind -inf)
    HB_HIP(hipMemsetD32Async((hipDeviceptr_t)ceil_i, 0xFFFFFFFFu, (size_t)nqp, s));
    const int out_metric = c.score_out ? 0 : ix->metric;
    double knn_ms = 0.0;
    int rc = 0;
    for (int col0 = 0; col0 < k && !rc; col0 += 256) {
        const int kp = std::min(256, k - col0);
        knn_call pass = c;
        pass.score_out = true;                               // ordering scores: what the next pass's ceiling compares with
        pass.ceil_s = col0 ? ceil_s : nullptr; pass.ceil_i = col0 ? ceil_i : nullptr;
        rc = knn_search(ix, pass, q_dev, nq, kp, 0, tmp_idx, tmp_sc);
        if (rc) break;
        if (c.timed) knn_ms += ix->last_knn_ms;
        bigk_place_kernel<<<dim3((unsigned)((nq * kp + 255) / 256)), dim3(256), 0, s>>>(tmp_idx, tmp_sc, nq, kp, k, col0, id_base, out_metric, c.q_aux,
                                                                                         out_idx, out_dist, ceil_s, ceil_i);
        HB_HIP(hipGetLastError());
    }
    if (c.timed) ix->last_knn_ms = knn_ms;
    return rc;
}

// ---- stage 1: which path serves the call, and the upkeep of the screen's two lazy copies of the bank (hbird_mirror.h) --------------------------------
struct knn_path {
    bool f16 = false;          // the candidate pass (the final decision: the upkeep below may still turn it off)
    int why = HB_WHY_EXPLICIT_FP32;
    bool automatic = false, wide_first = false;
    int how16 = HB_F16_CHAIN;
    bool centred = false;      // this pass runs on the centred copy
    int64_t fell_back = 0;     // (fp32) queries that count as fallbacks though no pass looked at them: the adaptive skip, an overflowed copy
};
static int knn_choose_path(hb_index* ix, const knn_call& c, int64_t nq, int k, knn_path* out) {
    knn_path& p = *out;
    const bool ceil = c.ceil_s != nullptr;      // a later pass of a search with k > 256: pools, the LDS-staged kernel's CEIL instantiation
    // fp16 mode 2 (what the plugin's use_fp16=True selects): the candidate pass only where it pays.  Its fixed costs are per query
    // (fp16 query tiles, re-rank of k' = 2k candidates, a second merge) and per search (the phases' launches and floor kernels), what it
    // saves is proportional to the matrix work rows x queries x D: the pass runs from rows x queries x D >= 1.5e10 x (k' / 64)^2 on, and
    // never below 4,096 rows.  Whole searches, fp32 / use_fp16 ms, same box, after round 4's changes (tools/exp_fp16_crossover.py): 196 x 384
    // queries: 65 k rows 0.28 / 0.34, 131 k 0.47 / 0.45, 1 M 1.93 / 0.95; 784 x 384: 16 k 0.28 / 0.34, 32 k 0.46 / 0.46, 65 k 0.64 / 0.51; 3,136 x
    // 384: 8 k 0.41 / 0.45, 16 k 0.65 / 0.47; 1,369 x 768: 4 k 0.30 / 0.23, 16 k 0.59 / 0.48; 12,544 x 384: 4 k 0.61 / 0.52, 50 k 3.9 / 1.5, 1 M
    // 69.3 / 10.6; 21,904 x 768: 4 k 1.43 / 1.09, 1 M 242.7 / 34.3; k = 90, 12,544 x 384: 16 k 1.74 / 2.04, 32 k 3.00 / 2.49, 1 M 70.4 / 13.8.
    // (Until round 4: at least 16,384 rows and rows x queries >= 2^27.)  Same results either way.
    const int esc = c.esc;
    // Which searches take the candidate pass is hb_screen_choose's decision (hbird_calibrate.cpp, with CPU tests): states 1 / 2 by the rule above;
    // the AUTOMATIC state (what a new index starts in) like state 2, but only for big searches -- from the 30,000 stages per workgroup at which the
    // fp32 kernels stamp and calibrate (below) --, on an index whose fp32 kernel the caller has not steered, and where the fp16 copy fits.
    hb_screen_in sin;
    sin.setting = c.fp16; sin.pinned = ix->fp32_pinned != 0; sin.env_off = ix->screen_env_off != 0; sin.k = k; sin.ceiling = ceil;
    sin.rows = ix->ntotal; sin.nq = nq; sin.d = ix->d; sin.overflow = ix->copy16.overflow != 0;
    sin.stages_per_wg = hb_stages_per_wg((nq + HB_QT - 1) / HB_QT, (ix->ntotal + HB_BT - 1) / HB_BT, hb_knn_workgroups(ix->force_G, ix->num_cu), ix->g8);
    sin.have_copy = ix->copy16.m.has(ix->cap_rows);
    sin.declined = ix->copy16.m.declined_at(ix->cap_rows);
    sin.bank_b = (uint64_t)ix->cap_rows * ix->dp * 4; sin.copy_b = (uint64_t)ix->cap_rows * ix->dp16 * 2;
    p.automatic = c.fp16 == HB_FP16_AUTO;
    p.f16 = hb_screen_choose(sin, &p.why);
    if (p.f16 && p.automatic && !sin.have_copy && nq > 0 && ix->ntotal > 0) {      // the copy has to be made: only where it leaves the device room
        ix->copy16.drop();      // (the bank grew: the old copy goes first)
        size_t free_b = 0, total_b = 0;
        HB_HIP(hipMemGetInfo(&free_b, &total_b));
        sin.mem_known = true; sin.free_b = free_b; sin.total_b = total_b;
        p.f16 = hb_screen_choose(sin, &p.why);
        if (!p.f16) ix->copy16.m.declined(ix->cap_rows);
    }
    // ADAPTIVE use (mode 2, round 6): on a bank whose neighbours sit closer together than fp16 can tell apart -- token worlds with little
    // noise: profiles/r06/final/fp16_cliff_*.json -- most certificates fail, and passes that certify nothing are pure overhead.  The index keeps
    // moving averages of the share of queries that failed the first certificate (r1) and of the share that reached the fp32 kernel (r12):
    // r12 > 1/2 -> the fp32 kernel right away; r1 > 1/2 -> the first pass is skipped, ONE pass with k' = 256 serves all queries; every 16th
    // search walks the whole chain again, so a bank (or a query stream) that changes is noticed.  Same bits on every path.
    if (p.f16 && esc == 0 && (c.fp16 == 2 || p.automatic) && ix->fp16_escalation == 0) {       // (the policy itself: hbird_calibrate.cpp, with CPU tests)
        p.how16 = hb_f16_choose(*c.adapt);
        if (p.how16 == HB_F16_FP32) { p.f16 = false; p.fell_back = nq; p.why = HB_WHY_ADAPTIVE; }
        else if (p.how16 == HB_F16_WIDE_FIRST) p.wide_first = true;
    }
    return 0;
}

// Bring the fp16 copy of the bank fragment tiles up to date; may turn f16 off (with its reason).  A finite value beyond the fp16 range
// (|x| > 65504) turns into inf there and the scores into inf / NaN, which the exactness certificate cannot bound: such a bank stays on the
// fp32 kernel (every query counts as a fallback)
static int knn_fp16_copy_upkeep(hb_index* ix, bool automatic, int64_t nq, hipStream_t s0, knn_path& path) {
    bool& f16 = path.f16;
    int& why = path.why;
    hb_fp16_copy& copy = ix->copy16;
    if (!copy.flag) { if (copy.flag.ensure(4, HB_GROW_EXACT)) return -1; HB_HIP(hipMemsetAsync(copy.flag, 0, 4, s0)); }
    if (!copy.m.has(ix->cap_rows)) {      // (the bank grew, or the allocation is about to be repeated)
        // states 1 / 2: the caller asked for the copy, no memory for it is the search's error.  Automatic: the copy only buys speed, so an
        // allocation that fails all the same (the device filled up since hipMemGetInfo) is remembered for this capacity and the fp32 kernel answers
        if (copy.make(ix->cap_rows, (size_t)ix->dp16 * 2, automatic)) {
            if (!automatic) return -1;
            f16 = false; why = HB_WHY_MEMORY;
        } else if (hipMemsetAsync(copy.tiles, 0, (size_t)ix->cap_rows * ix->dp16 * 2, s0) != hipSuccess) {
            copy.drop();
            return hb_fail("hb_index_search: zeroing the fp16 copy of the bank failed: " + std::string(hipGetErrorString(hipGetLastError())));
        }
    }
    if (f16 && copy.m.behind(ix->ntotal)) {
        int64_t rt0 = 0, n_rt = 0;
        copy.m.pending(ix->ntotal, &rt0, &n_rt);
        // (hb_index_set_fp16_centre: the rows as fl32(b - mu) with their per-row term, hbird_f16_centre.hip; a bank without a usable mean: the plain copy)
        int centred = 0;
        if (ix->fp16_centre && hb_centre_convert(ix, s0, &centred)) return -1;
        if (!centred && hb_launch_tiles_to_f16(ix->tiles, ix->g8, copy.tiles.as<_Float16>(), ix->dp16 / 16, n_rt, rt0, copy.flag, s0)) return -1;
        copy.m.converted(ix->ntotal);
        HB_HIP(hipMemcpyAsync(&copy.overflow, copy.flag, 4, hipMemcpyDeviceToHost, s0));
        HB_HIP(hipStreamSynchronize(s0));
    }
    if (f16 && copy.overflow) {
        f16 = false; why = HB_WHY_OVERFLOW; path.fell_back = nq;
        if (automatic) copy.drop();      // (nobody asked for this copy, and the flag is sticky: hb_screen_choose keeps the bank on the fp32 kernel without it)
    }
    return 0;
}
// ... and the row-major fp32 copy for the re-rank (hbird_knn_f16.hip).  Whether an automatic index gets one: hb_rerank_copy_choose
// (hbird_calibrate.cpp); a copy found not to fit is not asked about again until the capacity changes or the setting is set again
static int knn_row_copy_upkeep(hb_index* ix, hipStream_t s0) {
    if (ix->rerank_copy == 2) return 0;
    hb_row_copy& copy = ix->row_copy;
    const int rs = (ix->g8 * 8 + 31) / 32 * 32;
    if (copy.rows && !copy.has(ix->cap_rows, rs)) copy.drop();
    if (!copy.rows && (ix->rerank_copy == 1 || !copy.m.declined_at(ix->cap_rows))) {
        size_t free_b = 0, total_b = 0;
        HB_HIP(hipMemGetInfo(&free_b, &total_b));
        copy.m.declined(ix->cap_rows);     // (cleared when the copy is made; an allocation that fails all the same just means no copy -- unless the caller asked for it)
        if (hb_rerank_copy_choose(ix->rerank_copy, (uint64_t)ix->cap_rows * ix->dp * 4, (uint64_t)ix->cap_rows * rs * 4, free_b, total_b) &&
            !copy.make(ix->cap_rows, rs) && ix->rerank_copy == 1) return hb_fail("hb_index_search: no memory for the re-rank copy of the bank");
    }
    if (copy.rows && copy.m.behind(ix->ntotal)) {
        int64_t rt0 = 0, n_rt = 0;
        copy.m.pending(ix->ntotal, &rt0, &n_rt);
        if (hb_launch_tiles_to_row_copy(ix->tiles, ix->g8, copy.rows, rs, n_rt, rt0, s0)) return -1;
        copy.m.converted(ix->ntotal);
    }
    return 0;
}

// ---- stage 2: the work list of the plan, built where the cached one does not serve, and its device copy ---------------------------------
struct knn_work_list {
    const hb_schedule* sc = nullptr;
    double shares[8] = {1, 1, 1, 1, 1, 1, 1, 1};      // the GROUP shares the list was built with
    // device copy: [segs][wg_off][qt_off][qt_slots][wg_member][phase_bounds]
    const hb_seg* segs = nullptr;
    const int *wg_off = nullptr, *qt_off = nullptr, *qt_slots = nullptr, *wg_member = nullptr, *phase_bounds = nullptr;
    int n_phases = 1;          // 1: a single launch (lists; pools with too little work per workgroup)
    // this launch's share of every block's segments: [phase_begin(p)[b], phase_end(p)[b]) of the block's list
    const int* phase_begin(int p) const { return p == 0 ? wg_off : phase_bounds + (size_t)(p - 1) * sc->G; }
    const int* phase_end(int p) const { return p == n_phases - 1 ? wg_off + 1 : phase_bounds + (size_t)p * sc->G; }
};
static int knn_get_work_list(hb_index* ix, int esc, const hb_knn_plan& p, hipStream_t s, knn_work_list* out) {
    knn_work_list& wl = *out;
    static const double equal_shares[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    // (shares divided by their mean: eight equal shares of any size are the equal list, which is cached as such)
    if (p.balance) {
        double shares_n[8];
        double mean = 0.0;
        bool uneven = false;
        // calibrated shares belong to the physical XCDs: group g (blocks equal to g mod 8) gets the share of the XCD it was last seen on
        const hb_index::xcd_cal& xc = ix->xcal[p.fam];
        for (int x = 0; x < 8; ++x) mean += xc.w[x] / 8.0;
        for (int g = 0; g < 8; ++g) { shares_n[g] = xc.w[ix->xcd_balance == 0 ? xc.perm[g] : g] / mean; uneven = uneven || std::fabs(shares_n[g] - 1.0) > 1e-9; }
        if (uneven) std::copy(shares_n, shares_n + 8, wl.shares);
    }
    const double* shares = wl.shares;
    hb_schedule& sc = esc == 0 ? ix->sched : ix->sched_esc;      // (the nested searches of uncertified queries keep a list of their own: the caller's stays cached)
    hb_dev<char>& sched_dev = esc == 0 ? ix->sched_dev : ix->sched_esc_dev;
    const int nqt = p.nqt, nbt = p.nbt, G = p.G;
    // (a filled list's leftover query tiles get more slots: only as many as the floors between the phases and the merge take, hb_fill_slot_limit)
    const int fill_limit = p.filled ? hb_fill_slot_limit(p.klw, p.kc, p.phased) : 0;
    const bool rebuilt = !(sc.nqt == nqt && sc.nbt == nbt && sc.panel == p.panel && sc.cq == p.cq && sc.cb == p.cb && sc.phased == p.phased &&
                           sc.xcd_share == p.xs && sc.fill_asked == p.filled && sc.fill_slot_limit == fill_limit && (sc.G == G || (long long)nqt * nbt < G) &&
                           (sc.xcd_w.empty() ? std::equal(shares, shares + 8, equal_shares) : std::equal(shares, shares + 8, sc.xcd_w.begin())));
    if (rebuilt) { hb_build_schedule(nqt, nbt, G, p.panel, sc, p.cq, p.cb, p.phased, p.xs, shares, p.filled, fill_limit); ++ix->sched_builds; }
    const struct { const void* data; size_t bytes; } part[6] = {{sc.segs.data(), sc.segs.size() * sizeof(hb_seg)}, {sc.wg_off.data(), sc.wg_off.size() * 4},
        {sc.qt_off.data(), sc.qt_off.size() * 4}, {sc.qt_slots.data(), sc.qt_slots.size() * 4}, {sc.wg_member.data(), sc.wg_member.size() * 4},
        {sc.phase_bounds.data(), sc.phase_bounds.size() * 4}};
    size_t off[7] = {0};
    for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + al256(part[i].bytes);
    const bool need_upload = rebuilt || sched_dev.bytes < off[6];
    if (sched_dev.ensure(off[6], HB_GROW_QUARTER)) return -1;
    if (need_upload) {
        for (int i = 0; i < 6; ++i) HB_HIP(hipMemcpyAsync(sched_dev + off[i], part[i].data, part[i].bytes, hipMemcpyHostToDevice, s));
        HB_HIP(hipStreamSynchronize(s));   // host vectors may be rebuilt by the next call
    }
    auto ints = [&](int i) { return sched_dev.as<const int>(off[i]); };
    wl.sc = &sc; wl.segs = sched_dev.as<const hb_seg>();
    wl.wg_off = ints(1); wl.qt_off = ints(2); wl.qt_slots = ints(3); wl.wg_member = ints(4); wl.phase_bounds = ints(5);
    wl.n_phases = (int)sc.phase_clock.size() + 1;
    return 0;
}

// ---- stage 3: `state` carved into the kernels' arguments: lists / pools, floors, progress words, stamps ---------------------------------
struct knn_workspace {
    knn_args a;                // (wg_off / wg_end: set per phase by the runner's launch)
    size_t state_aux = 0;      // bytes of the pools' fill counts (and of their thresholds)
    size_t prog_bytes = 0, stamp_bytes = 0;
};
static int knn_carve_workspace(hb_index* ix, const knn_call& c, const hb_knn_plan& p, const knn_work_list& wl, int64_t nq, int k, hipStream_t s,
                               knn_workspace* out) {
    const hb_schedule& sc = *wl.sc;
    const int nqt = p.nqt, klw = p.klw, esc = c.esc;
    const size_t state_half = (size_t)sc.n_slots * HB_QT * klw * 4;
    const size_t state_aux = p.wide ? (size_t)sc.n_slots * HB_QT * 4 : 0;   // pools: fill counts + thresholds
    const size_t floor_bytes = (size_t)nqt * HB_QT * 4 * 17;              // shared threshold floors, one per query, + 16 quota-floor keys per query
    const size_t prog_bytes = ((size_t)std::max(1, sc.n_clusters) * HB_CLUSTER_MAX + 1) * HB_CLUSTER_LINE * 4;   // progress words, a line each, + statistics
    const size_t stamp_bytes = (size_t)sc.G * 32;                       // per-block {start, end, XCC id} stamps of the last kNN launch with its shader-cycle counts (wg_stamp, hbird_knn_dev.h)
    if (ix->state.ensure(2 * state_half + 2 * state_aux + floor_bytes + prog_bytes + stamp_bytes, HB_GROW_QUARTER)) return -1;
    out->state_aux = state_aux; out->prog_bytes = prog_bytes; out->stamp_bytes = stamp_bytes;
    char* const floors = ix->state + 2 * state_half + 2 * state_aux;
    knn_args& a = out->a;
    // (a nested search of uncertified queries neither stamps nor counts as "the last launch": hb_index_kernel_clock / hb_index_wg_stamps describe the
    // caller's search, as hb_index_schedule_info does)
    a.wg_stamp = esc == 0 && (c.timed || p.calibrated) ? reinterpret_cast<unsigned*>(floors + floor_bytes + prog_bytes) : nullptr;
    if (esc == 0) { ix->wg_stamp_dev = a.wg_stamp; ix->wg_stamp_blocks = sc.G; }
    if (a.wg_stamp) HB_HIP(hipMemsetAsync(a.wg_stamp, 0, stamp_bytes, s));   // a block that never stamps reads 0 / 0 (hb_stamps_summarise)
    a.bank_tiles = ix->tiles; a.binit = ix->binit; a.q_tiles = ix->q_tiles;
    a.ceil_s = c.ceil_s; a.ceil_i = c.ceil_i; a.segs = wl.segs; a.wg_off = wl.wg_off; a.wg_end = a.wg_off + 1;
    a.state_s = ix->state.as<float>();
    a.state_i = ix->state.as<unsigned>(state_half);
    a.g8 = ix->g8; a.k = k; a.klw = klw;
    a.state_cnt = ix->state.as<int>(2 * state_half);
    a.state_thr = ix->state.as<float>(2 * state_half + state_aux);
    a.gthr = reinterpret_cast<unsigned*>(floors);
    a.qfl = a.gthr + (size_t)nqt * HB_QT;
    HB_HIP(hipMemsetD32Async((hipDeviceptr_t)a.gthr, 0x007FFFFF, (size_t)nqt * HB_QT * 17, s));   // key(-inf)
    // the padding queries of the last query tile (zero vectors: every row scores the same) start from key(+inf): nothing ever passes
    // their threshold.  Without it a slot's first tile appended all 256 tied rows for each of them and compacted their pools on the spot
    // (50,176 x 384 x 21,904 queries, 112 padding queries, pools: 943 us for a one-tile phase that takes 136 us with 21,760 queries)
    if (nq < (int64_t)nqt * HB_QT) HB_HIP(hipMemsetD32Async((hipDeviceptr_t)(a.gthr + nq), 0xFF800000u, (size_t)((int64_t)nqt * HB_QT - nq), s));
    // a nested search of uncertified queries starts from what the pass before it found out (hb_rerank_seeds): per query a score that the
    // rows which can still matter reach
    if (esc != 0 && c.seed) {
        seed_from_scores_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s>>>(c.seed, nq, a.gthr);
        HB_HIP(hipGetLastError());
    }
    a.wg_member = wl.wg_member; a.prog = reinterpret_cast<int*>(floors + floor_bytes);
    a.cl = sc.cq * sc.cb; a.lag = p.lag;      // (soft-sync lag in stages: hb_knn_plan_clusters)
    a.cl_stats = a.prog + (size_t)std::max(1, sc.n_clusters) * HB_CLUSTER_MAX * HB_CLUSTER_LINE;
    ix->cl_stats_dev = a.cl > 1 ? a.cl_stats : nullptr;
    if (a.cl > 1) HB_HIP(hipMemsetAsync(a.prog, 0, prog_bytes, s));
    return 0;
}

// ---- stage 4: the phases of one search, for both kernel families ------------------------------------------------------------------------
// between two phases of a pool search: the kk-th best of all rows seen so far becomes every slot's floor -- straight from the pools
// where a query tile's pools fit the floor kernel's LDS, else through the merge (few queries against a big bank: many slots)
static int knn_seed_floors(hb_index* ix, const knn_args& a, const knn_work_list& wl, int nqt, int klw, int64_t nq, int kk, int64_t* scratch_idx,
                           float* scratch_dist, hipStream_t s) {
    const hb_schedule& sc = *wl.sc;
    const size_t per_wave = (size_t)sc.max_slots_per_qt * klw;
    // (up to 144 KiB of the CU's 160: 32 slots per query tile x pools of 256, 16 x 512 -- the merge path below costs a phase boundary
    // ten times as much: 10 M x 768, k = 90 with 16 slots per query tile: 2.9 -> 44.7 ms per search, profiles/r04/cluster_tail_rows_ab.txt)
    if (per_wave * 16 <= 144 * 1024) {
        if (per_wave * 16 > 48 * 1024 && hb_ensure_dyn_lds((const void*)pool_floor_kernel, 144 * 1024)) return -1;
        pool_floor_kernel<<<dim3((unsigned)((nq + 3) / 4)), dim3(256), per_wave * 16, s>>>(a.state_s, a.state_cnt, a.state_thr, wl.qt_off, wl.qt_slots, nq, kk,
                                                                                           klw, (int)per_wave, a.gthr);
        HB_HIP(hipGetLastError());
        return 0;
    }
    if (launch_merge(ix, a.state_s, a.state_i, a.state_cnt, a.state_thr, wl.qt_off, wl.qt_slots, sc.max_slots_per_qt, nqt, nq, kk, klw, 0, 0, nullptr,
                     scratch_idx, scratch_dist, s)) return -1;
    seed_floors_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s>>>(scratch_idx, scratch_dist, nq, kk, a.gthr);
    HB_HIP(hipGetLastError());
    return 0;
}

// launch(begin, end) starts one phase: begin[b] .. end[b] of block b's segments.  kk and the scratch lists are what the floors between two
// phases are taken from (the kk-th best of all rows seen so far); kk is also the k of the calibration's shape key.
template <class Launch>
static int knn_run_phases(hb_index* ix, const knn_call& c, const hb_knn_plan& p, const knn_work_list& wl, const knn_workspace& ws, int64_t nq, int kk,
                          int64_t* scratch_idx, float* scratch_dist, hipStream_t s, Launch launch) {
    const knn_args& a = ws.a;
    if (c.timed) HB_HIP(hipEventRecord(ix->ev0, s));
    if (wl.n_phases > 1) {   // (pools only) slots that start in a later phase must read as empty pools in the merges between the phases
        HB_HIP(hipMemsetAsync(a.state_cnt, 0, ws.state_aux, s));
        HB_HIP(hipMemsetD32Async((hipDeviceptr_t)a.state_thr, 0xFF800000u, ws.state_aux / 4, s));
    }
    for (int ph = 0; ph < wl.n_phases; ++ph) {
        if (launch(wl.phase_begin(ph), wl.phase_end(ph))) return -1;
        if (ph + 1 < wl.n_phases) {   // the kk-th best ORDERING score of all rows seen so far -> every slot's floor
            if (knn_seed_floors(ix, a, wl, p.nqt, p.klw, nq, kk, scratch_idx, scratch_dist, s)) return -1;
            if (a.cl > 1) HB_HIP(hipMemsetAsync(a.prog, 0, ws.prog_bytes - HB_CLUSTER_LINE * 4, s));   // progress words (not the statistics)
        }
    }
    if (c.timed) HB_HIP(hipEventRecord(ix->ev1, s));
    if (p.calibrated && c.esc == 0 && hb_xcd_collect(ix, p.fam, a.wg_stamp, *wl.sc, wl.shares, wl.n_phases, p.nqt, p.nbt, kk, s, p.auto_cluster)) return -1;
    return 0;
}
// ... and, once whatever follows the kernels has been launched behind them, their time
static int knn_read_time(hb_index* ix, const knn_call& c) {
    if (!c.timed) return 0;
    HB_HIP(hipEventSynchronize(ix->ev1));
    float ms = 0.f;
    HB_HIP(hipEventElapsedTime(&ms, ix->ev0, ix->ev1));
    ix->last_knn_ms = ms;
    return 0;
}

// ---- stage 5: the fp16 path: candidate pass, exact re-rank, certificates, re-search of what failed -------------------------------------
// workspace of one level: [certificates nq + 64][exact k-th scores nq][floors for a second pass nq] and, once the failures are
// known, [their rows][queries][aux][floors][ids][distances]
// -- a caller's search keeps it in fb, the second fp16 pass in fb1 (the fp32 search of what is left has no failures of its own)
// (the layout itself: hb_level_layout, hbird_report.h, which the read-outs compute it from as well)
struct knn_level_buf : hb_level_layout {
    hb_devbuf& buf;
    knn_level_buf(hb_index* ix, int esc, int64_t nq) : hb_level_layout(nq), buf(esc == 0 ? ix->fb : ix->fb1) {}
    float* kth() const { return buf.as<float>(o_kth); }
    float* flo() const { return buf.as<float>(o_flo); }
};

// The queries `bad` of this level are searched again: gathered, re-tiled, searched by a nested call, scattered into the outputs.
static int knn_research_failures(hb_index* ix, const knn_call& c, const knn_path& path, const hb_knn_plan& p, const knn_work_list& wl, const knn_workspace& ws,
                                 const std::vector<int64_t>& bad, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist,
                                 hipStream_t s) {
    const int esc = c.esc;
    const int64_t nf = (int64_t)bad.size();
    const knn_level_buf lv(ix, esc, nq);
    hb_devbuf& fbuf = lv.buf;
    const size_t o_rows = lv.o_rows;
    // the second pass needs k' = 256 > the first one's, a bank worth a candidate pass, and is not repeated
    const bool again16 = esc == 0 && ix->fp16_escalation == 0 && p.kc < 256 && ix->ntotal >= 4096;
    // An excluding search: a floor-seeded fp32 search knows nothing of groups, so what the second pass cannot take is handed back to the caller
    // (hb_index_search_excluding: the rungs, on these queries only)
    if (c.groups && !again16) {
        std::vector<int64_t> left;
        for (int64_t b : bad) left.push_back(c.excl_orig ? c.excl_orig[b] : b);
        c.rep->left_to_rungs(std::move(left));
        return 0;
    }
    const size_t o_q = o_rows + al256((size_t)nf * 8), o_aux = o_q + al256((size_t)nf * ix->d * 4), o_seed = o_aux + al256((size_t)nf * 8),
                 o_idx = o_seed + al256((size_t)nf * 4), o_dist = o_idx + al256((size_t)nf * k * 8), o_qg = o_dist + al256((size_t)nf * k * 4),
                 tot2 = o_qg + (c.groups ? al256((size_t)nf * 4) : 0);
    if (fbuf.ensure_keep(tot2, HB_GROW_QUARTER, o_rows, s)) return -1;      // (kept: the certificates and the seeds of this level)
    const float *kth = lv.kth(), *flo = lv.flo();      // (after the move)
    int64_t* d_rows = fbuf.as<int64_t>(o_rows);
    float* d_q = fbuf.as<float>(o_q);
    float* d_aux = fbuf.as<float>(o_aux);
    float* d_seed = fbuf.as<float>(o_seed);
    int64_t* d_fi = fbuf.as<int64_t>(o_idx);
    float* d_fd = fbuf.as<float>(o_dist);
    HB_HIP(hipMemcpyAsync(d_rows, bad.data(), (size_t)nf * 8, hipMemcpyHostToDevice, s));
    if (hb_launch_gather_rows(q_dev, nq, ix->d, d_rows, nf, d_q, s)) return -1;
    if (hb_launch_gather_rows(again16 ? flo : kth, nq, 1, d_rows, nf, d_seed, s)) return -1;
    if (hb_launch_rows_to_tiles(d_q, nf, ix->d, ix->dp, 0, ix->q_tiles, nullptr, nullptr, ix->metric, 0, 0, s)) return -1;
    // What the nested search shares with this one THROUGH THE INDEX (everything else it is told by its knn_call):
    //   q_tiles  overwritten just above with the re-searched queries' tiles (this level has no further use for its own);
    //   state    taken for the nested search's own pools, and it may move: the candidate launch's stamps go aside first (stamp_keep);
    //   sched    the nested levels keep ONE work list of their own (sched_esc), so the caller's stays cached;
    //   fb       this level's workspace, the second fp16 pass's is fb1 (knn_level_buf).
    if (esc == 0 && ws.a.wg_stamp) {
        if (ix->stamp_keep.ensure(ws.stamp_bytes, HB_GROW_EXACT)) return -1;      // (32 bytes per workgroup of the candidate launch)
        HB_HIP(hipMemcpyAsync(ix->stamp_keep, ws.a.wg_stamp, ws.stamp_bytes, hipMemcpyDeviceToDevice, s));
        ix->wg_stamp_dev = ix->stamp_keep;
    }
    int rc = hb_launch_query_aux(d_q, nf, ix->d, d_aux, d_aux + nf, s);      // chain ||q||^2 of the re-searched queries (L2 distances)
    knn_call nested;
    nested.rep = c.rep; nested.adapt = c.adapt;
    nested.esc = again16 ? 1 : 2; nested.seed = d_seed;
    nested.fp16 = again16 ? 1 : 0; nested.timed = false; nested.q_aux = d_aux; nested.score_out = c.score_out;
    if (c.groups) {      // (again16) the second pass drops the same groups: gathered with the queries
        int32_t* d_qg = fbuf.as<int32_t>(o_qg);
        if (!rc) rc = hb_launch_gather_groups(c.groups, nq, d_rows, nf, d_qg, s);
        nested.groups = d_qg; nested.excl_orig = bad.data();
    }
    if (again16) c.rep->sent_to_second_pass(bad, o_seed, c.groups ? o_qg : 0);      // (the second pass merges into ix->cand)
    else c.rep->reached_fp32(nf, esc);
    if (!rc) rc = knn_search(ix, nested, d_q, nf, k, id_base, d_fi, d_fd);
    if (rc) return -1;
    if (esc == 0 && !c.groups) hb_f16_observe(*c.adapt, path.how16, nq, nf, c.rep->fallbacks);      // (an excluding search's failures say nothing about plain ones)
    if (hb_launch_scatter_rows(d_rows, nf, k, d_fi, d_fd, out_idx, out_dist, s)) return -1;
    HB_HIP(hipStreamSynchronize(s));         // `bad` and the workspace are reused by the next call
    return 0;
}

static int knn_search_f16(hb_index* ix, const knn_call& c, const knn_path& path, const hb_knn_plan& p, const knn_work_list& wl, const knn_workspace& ws,
                          const float* q_dev, int64_t nq, int k, int64_t id_base, int out_metric, int64_t* out_idx, float* out_dist,
                          hipStream_t s) {
    const knn_args& a = ws.a;
    const hb_schedule& sc = *wl.sc;
    const int esc = c.esc, kc = p.kc, klw = p.klw, nqt = p.nqt;
    const bool centred = path.centred;
    // fp16 copy of the query fragment tiles (the bank's is up to date: top of this function)
    const int64_t nqp = (int64_t)nqt * HB_QT;
    if (ix->q16.ensure((size_t)nqp * ix->dp16 * 2, HB_GROW_QUARTER)) return -1;
    // centred: fp16 tiles of q - t mu, c_q and ||q - t mu|| per query; a caller's search also derives t and, from it, the rows' init values
    hb_centre_view cview{nullptr, nullptr, nullptr};
    if (centred) { if (hb_centre_queries(ix, nq, esc == 0, ix->q16.as<_Float16>(), &cview, s)) return -1; }      // (whose queries these are: the level's transition below)
    else if (hb_launch_tiles_to_f16(ix->q_tiles, ix->g8, ix->q16.as<_Float16>(), ix->dp16 / 16, nqp / 32, 0, nullptr, s)) return -1;
    if (ix->cand.ensure((size_t)nq * kc * 12, HB_GROW_QUARTER)) return -1;
    int64_t* cand_idx = ix->cand.as<int64_t>();
    float* cand_dist = ix->cand.as<float>((size_t)nq * kc * 8);
    knn16_args h;
    h.wg_stamp = a.wg_stamp;
    h.bank16 = ix->copy16.tiles.as<const _Float16>(); h.binit = centred ? ix->copy16.centre.init16 : ix->binit; h.q16 = ix->q16.as<const _Float16>(); h.segs = a.segs; h.wg_off = a.wg_off; h.wg_end = a.wg_end;
    h.state_s = a.state_s; h.state_i = a.state_i; h.g16 = ix->dp16 / 16; h.k = kc; h.klw = klw;
    h.state_cnt = a.state_cnt; h.state_thr = a.state_thr; h.gthr = a.gthr;
    h.wg_member = a.wg_member; h.prog = a.prog; h.cl = a.cl; h.lag = a.lag; h.cl_stats = a.cl_stats;
    if (knn_run_phases(ix, c, p, wl, ws, nq, kc, cand_idx, cand_dist, s, [&](const int* begin, const int* end) {
            h.wg_off = begin; h.wg_end = end;
            return hb_knn_f16_launch(h, sc.G, s);
        })) return -1;
    // the tail: merge to candidates, exact re-rank with the certificates, and the certificates back on the host
    if (launch_merge(ix, a.state_s, a.state_i, a.state_cnt, a.state_thr, wl.qt_off, wl.qt_slots, sc.max_slots_per_qt, nqt, nq, kc, klw, 0, 0, nullptr,
                     cand_idx, cand_dist, s)) return -1;
    const knn_level_buf lv(ix, esc, nq);
    if (lv.buf.ensure(lv.o_rows, HB_GROW_QUARTER)) return -1;
    unsigned char* cert = lv.buf.as<unsigned char>();
    float *kth = lv.kth(), *flo = lv.flo();
    HB_HIP(hipMemsetD32Async((hipDeviceptr_t)kth, 0xFF800000u, (lv.o_rows - lv.o_kth) / 4, s));    // -inf: no seed (a query with fewer than k candidates)
    const float* q_aux = c.q_aux;
    const hb_rerank_args ra{ix->binit, ix->d, q_dev, q_aux, cand_idx, cand_dist, q_aux + nq, ix->bmax, cert, kc, nq, k, id_base, ix->metric, out_metric,
                            ix->ntotal, out_idx, out_dist, hb_rerank_seeds{esc == 1 ? c.seed : nullptr, kth, flo}, cview};
    const bool row_copy = ix->row_copy.rows && ix->rerank_copy != 2 && !ix->row_copy.m.behind(ix->ntotal);
    // an excluding search: the re-rank that drops every query's group among its candidates (hbird_exclude_screen.hip; from the tiles)
    if (c.groups ? hb_launch_excl_screen_rerank(ra, ix->tiles, ix->g8, ix->row_groups, ix->row_groups_n, c.groups, s)
                 : hb_launch_rerank(ra, ix->tiles, ix->g8, row_copy ? ix->row_copy.rows : nullptr, ix->row_copy.rs, s)) return -1;
    if (knn_read_time(ix, c)) return -1;
    // Queries whose certificate failed are searched again.  ESCALATION (round 6): first by a second fp16 pass with k' = 256 candidates
    // (the certificate compares the exact k-th best with the fp16 score of rank k': four times the ranks apart) whose pools start from
    // the floor `kth - 1.001 E` -- every row that can still matter scores above it in fp16, few others do, so the pass appends little and
    // a list that does not fill up is complete by construction; only what fails again goes to the exact fp32 kernel, which starts from
    // the exact k-th best found so far as its floor.  A failing query used to cost a share of a whole-bank fp32 search (10 M x 768: 27 ms
    // per started tile of 256 queries; 5 % failing queries = +45 % on the step): the second pass costs a twentieth of that per query.
    std::vector<unsigned char> hc((size_t)nq);
    HB_HIP(hipMemcpyAsync(hc.data(), cert, (size_t)nq, hipMemcpyDeviceToHost, s));
    HB_HIP(hipStreamSynchronize(s));
    std::vector<int64_t> bad;
    for (int64_t i = 0; i < nq; ++i) if (!hc[i]) bad.push_back(i);
    const int64_t nf = (int64_t)bad.size();
    // (cand, q16 and the certificates are complete: the stream is idle)
    if (esc == 0) c.rep->level0_finished(nq, kc, klw, centred, nf);
    else c.rep->level1_finished(nq, kc, klw, centred, nf);
    if (esc == 0 && nf == 0 && !c.groups) hb_f16_observe(*c.adapt, path.how16, nq, 0, 0);
    if (nf > 0 && knn_research_failures(ix, c, path, p, wl, ws, bad, q_dev, nq, k, id_base, out_idx, out_dist, s)) return -1;
    return 0;
}

// ---- ... and the fp32 path: the plan's kernel, the merge into the outputs -------------------------------------------------------------
static int knn_search_f32(hb_index* ix, const knn_call& c, const hb_knn_plan& p, const knn_work_list& wl, const knn_workspace& ws, int64_t nq, int k,
                          int64_t id_base, int out_metric, int64_t* out_idx, float* out_dist, hipStream_t s) {
    const hb_schedule& sc = *wl.sc;
    typedef void (*knn_fn)(knn_args);
    knn_fn fn = nullptr;
    int lds_bytes = KN_LDS_TOTAL;
    switch (p.kernel) {      // (which one and why: hb_knn_plan_kernel)
        case HB_KERNEL_LISTS: fn = knn_fused_kernel<false, false>; break;
        case HB_KERNEL_LISTS_COLD: fn = knn_fused_kernel<true, false>; lds_bytes = KN_LDS_TOTAL_COLD; break;
        case HB_KERNEL_POOLS: fn = knn_fused_kernel<false, true>; break;
        case HB_KERNEL_LISTS_CL: fn = knn_fused_kernel<false, false, true>; break;
        case HB_KERNEL_POOLS_CL: fn = knn_fused_kernel<false, true, true>; break;
        case HB_KERNEL_CEIL: fn = knn_fused_kernel<false, true, false, true>; break;
        default:      // HB_KERNEL_BD + ...: query fragments straight into registers (hbird_knn_bd.hip)
            fn = hb_knn_bd_kernel(p.wide, ws.a.cl > 1, p.small);
            lds_bytes = hb_knn_bd_lds_bytes(p.small && !p.wide);
    }
    if (hb_ensure_dyn_lds((const void*)fn, lds_bytes)) return -1;   // per (kernel, device)
    knn_args a = ws.a;
    // (between two phases the outputs serve as scratch)
    if (knn_run_phases(ix, c, p, wl, ws, nq, k, out_idx, out_dist, s, [&](const int* begin, const int* end) {
            a.wg_off = begin; a.wg_end = end;
            fn<<<dim3((unsigned)sc.G), dim3(HB_THREADS), lds_bytes, s>>>(a);
            HB_HIP(hipGetLastError());
            return 0;
        })) return -1;
    const float* qn2 = c.q_aux;   // [nq] chain ||q||^2 (valid for L2)
    const int* pool_cnt = p.wide ? a.state_cnt : nullptr;
    if (launch_merge(ix, a.state_s, a.state_i, pool_cnt, pool_cnt ? a.state_thr : nullptr, wl.qt_off, wl.qt_slots, sc.max_slots_per_qt, p.nqt, nq, k, p.klw,
                     id_base, out_metric, qn2, out_idx, out_dist, s)) return -1;
    return knn_read_time(ix, c);
}

// One search of at most 256 neighbours as a sequence of stages: path -> screen upkeep -> plan -> work list -> workspace -> the path's kernels.
static int knn_search(hb_index* ix, const knn_call& c, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist) {
    if (k < 1 || k > HB_MAX_K) return hb_fail("hb_index_search: k must be in [1, " + std::to_string(HB_MAX_K) + "] (faiss-gpu's limit, search_faiss.py:84-85)");
    if (k > 256) return hb_launch_knn_bigk(ix, c, q_dev, nq, k, id_base, out_idx, out_dist);
    hipStream_t s = ix->stream;
    const int esc = c.esc;
    if (esc == 0) c.rep->begin(c.groups != nullptr);
    knn_path path;
    if (knn_choose_path(ix, c, nq, k, &path)) return -1;
    if (path.f16 && nq > 0 && ix->ntotal > 0 && knn_fp16_copy_upkeep(ix, path.automatic, nq, s, path)) return -1;
    if (path.f16 && nq > 0 && ix->ntotal > 0 && knn_row_copy_upkeep(ix, s)) return -1;
    path.centred = path.f16 && ix->fp16_centre && ix->copy16.centre.active;
    if (c.groups && !path.f16) {      // an excluding search goes where a plain search at (nq, k) takes the candidate pass, and nowhere else
        if (esc != 0) return hb_fail("hb_index_search_excluding: the second pass of an excluding search left the fp16 screen");
        return 0;      // (the report says so: no candidate pass)
    }
    if (esc == 0) c.rep->path_chosen(!path.f16 ? HB_PATH_FP32 : path.wide_first ? HB_PATH_FP16_WIDE : HB_PATH_FP16_CHAIN, path.why, path.centred, path.fell_back);
    if (nq == 0) return 0;
    // score output (sharded searches): the ordering score goes out as it is, whatever the metric
    const int out_metric = c.score_out ? 0 : ix->metric;
    if (ix->ntotal == 0) {
        // empty index: every neighbour is missing (faiss returns -1 labels)
        std::vector<int64_t> hi((size_t)nq * k, -1);
        std::vector<float> hd((size_t)nq * k, out_metric == 1 ? INFINITY : -INFINITY);
        HB_HIP(hipMemcpyAsync(out_idx, hi.data(), hi.size() * 8, hipMemcpyHostToDevice, s));
        HB_HIP(hipMemcpyAsync(out_dist, hd.data(), hd.size() * 4, hipMemcpyHostToDevice, s));
        HB_HIP(hipStreamSynchronize(s));
        return 0;
    }
    // the plan (hbird_calibrate.cpp).  hb_xcd_calibrate runs BEFORE the cluster shape is chosen: it also decides whether the fp32 clusters stay
    hb_knn_plan_in pin;
    pin.f16 = path.f16; pin.wide_first = path.wide_first; pin.esc = esc; pin.ceil = c.ceil_s != nullptr;
    pin.k = k; pin.nq = nq; pin.ntotal = ix->ntotal; pin.g8 = ix->g8; pin.dp = ix->dp; pin.dp16 = ix->dp16; pin.num_cu = ix->num_cu;
    pin.force_G = ix->force_G; pin.force_panel = ix->force_panel; pin.force_cq = ix->force_cq; pin.force_cb = ix->force_cb; pin.variant = ix->variant;
    pin.small_limit = ix->small_limit; pin.phases_on = ix->phases_on; pin.xcd_balance = ix->xcd_balance; pin.xcd_share = ix->xcd_share; pin.sync_lag = ix->sync_lag;
    hb_knn_plan p;
    hb_knn_plan_shape(pin, p);
    if (p.calibrated && esc == 0) hb_xcd_calibrate(ix, p.fam);     // (nested searches run on the shares in use and leave the calibration alone)
    pin.cl_state = ix->xcal[0].cl_state; pin.cl_choice = ix->xcal[0].cl_choice;
    hb_knn_plan_clusters(pin, p);
    knn_work_list wl;
    if (knn_get_work_list(ix, esc, p, s, &wl)) return -1;
    hb_knn_plan_kernel(pin, wl.sc->G, p);
    knn_workspace ws;
    if (knn_carve_workspace(ix, c, p, wl, nq, k, s, &ws)) return -1;
    if (path.f16) return knn_search_f16(ix, c, path, p, wl, ws, q_dev, nq, k, id_base, out_metric, out_idx, out_dist, s);
    return knn_search_f32(ix, c, p, wl, ws, nq, k, id_base, out_metric, out_idx, out_dist, s);
}

// what a level-0 search reads of its queries: their fragment tiles in q_tiles, chain ||q||^2 and fp32 norms in q_aux
static int hb_prepare_queries(hb_index* ix, const float* q_dev, int64_t nq) {
    const int64_t nqp = (nq + HB_QT - 1) / HB_QT * HB_QT;
    if (ix->q_tiles.ensure((size_t)nqp * ix->dp * 4, HB_GROW_EXACT)) return -1;
    if (ix->q_aux.ensure((size_t)nq * 2 * 4, HB_GROW_EXACT)) return -1;
    if (hb_launch_rows_to_tiles(q_dev, nq, ix->d, ix->dp, 0, ix->q_tiles, nullptr, nullptr, ix->metric, 0, 0, ix->stream)) return -1;
    return hb_launch_query_aux(q_dev, nq, ix->d, ix->q_aux, ix->q_aux + nq, ix->stream);
}
// the level-0 call: a caller's search, by the index's settings, on the queries hb_prepare_queries took; it reports into *rep
static knn_call knn_level0_call(hb_index* ix, hb_search_report* rep, hb_f16_adapt* adapt) {
    knn_call c;
    c.fp16 = ix->fp16; c.timed = ix->time_kernels != 0; c.q_aux = ix->q_aux; c.score_out = ix->score_output != 0;
    c.rep = rep; c.adapt = adapt;
    return c;
}

// The caller-level entry of a plain search (q_tiles / q_aux prepared): the report is built here, handed down, and committed when the search is
// over -- the empty one if it failed.  A detached search writes the pair it was given and commits nothing.
static int hb_launch_knn(hb_index* ix, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist, hb_detached* detached) {
    if (detached) return knn_search(ix, knn_level0_call(ix, &detached->rep, &detached->adapt), q_dev, nq, k, id_base, out_idx, out_dist);
    hb_search_report rep;
    const int rc = knn_search(ix, knn_level0_call(ix, &rep, &ix->f16_adapt), q_dev, nq, k, id_base, out_idx, out_dist);
    return ix->commit(std::move(rep), rc);
}

int hb_search_device(hb_index* ix, const float* q_dev, int64_t nq, int k, int64_t id_base, int64_t* out_idx, float* out_dist, hb_detached* detached) {
    {
        hb_range r("hbird:query_tiles");
        if (hb_prepare_queries(ix, q_dev, nq)) return -1;
    }
    hb_range r("hbird:knn");
    return hb_launch_knn(ix, q_dev, nq, k, id_base, out_idx, out_dist, detached);
}

// An excluding search on the screen (hbird_internal.h): the level-0 call of a plain search at k -- query tiles and norms as hb_index_search
// prepares them -- with the queries' groups in its context.  The caller has checked 1 <= k <= 128, nq > 0, ntotal > 0 and the group table.
int hb_launch_knn_excluding(hb_index* ix, const float* q_dev, int64_t nq, int k, int64_t id_base, const int32_t* qgroups, int64_t* out_idx, float* out_dist,
                            hb_search_report* rep) {
    int rc = hb_prepare_queries(ix, q_dev, nq);
    if (!rc) {
        knn_call c = knn_level0_call(ix, rep, &ix->f16_adapt);
        c.groups = qgroups;
        rc = knn_search(ix, c, q_dev, nq, k, id_base, out_idx, out_dist);
    }
    return rc ? ix->commit(hb_search_report(), rc) : 0;
}
