// nr_free_bin.hip — the binning, planning and pruning kernels of the
// visibility-buffer raster (steps 1-3 of nr_tri_free.hip's head comment, the
// warm binning and its gate, the visible list's pruning, the visible plan and
// the key plan), each behind one host launch function (nr_free.h).
#include "nr_free.h"

#include <hip/hip_ext.h>

namespace nrtri {
namespace {

// Tile rectangle of a triangle, packed for the emit pass (16 bits per bound;
// NO_RECT: the triangle produces no fragment).
constexpr u64 NO_RECT = ~0ull;
__device__ __forceinline__ u64 pack_rect(int tx0, int tx1, int ty0, int ty1) {
    return (u64)(u32)tx0 | ((u64)(u32)tx1 << 16) | ((u64)(u32)ty0 << 32) | ((u64)(u32)ty1 << 48);
}

// REC (ordered batches): also the triangle's setup record for the ordered
// raster (write_ordered_record), formed once here instead of in every tile.
template <bool LDSH, bool REC = false>
__global__ __launch_bounds__(256) void k_free_count(const BinParams bp, u32* __restrict__ tile_cnt, int ntiles,
                                                    u64* __restrict__ rects, f64* __restrict__ rec = nullptr) {
    extern __shared__ u32 hist[];
    const int tid = threadIdx.x;
    const i64 base = (i64)blockIdx.x * 256 * TPT;
    // every triangle's positions first (in flight during the histogram's
    // zeroing): one round of load latency, not TPT
    f64 pxy[TPT][6];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        if (t < bp.src.n) load_tri_xy(bp.src.xy, t, pxy[k]);
    }
    // LDS histogram over the owned tile rows only (a sharded frame's share)
    const int hbins = bp.hrows * bp.tiles_x;
    if (LDSH) {
        for (int b = tid; b < hbins; b += 256) hist[b] = 0;
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        if (t >= bp.src.n) break;
        f64 sx[3], sy[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) nr_xform(bp.m, pxy[k][2 * v], pxy[k][2 * v + 1], sx[v], sy[v]);
        int tx0, tx1, ty0, ty1;
        const bool hit = tri_tiles(sx, sy, bp.W, bp.H, tx0, tx1, ty0, ty1);
        rects[t] = hit ? pack_rect(tx0, tx1, ty0, ty1) : NO_RECT;
        if (!hit) continue;
        if (REC) write_ordered_record(rec, t, sx, sy, bp.src.z);   // (hit: finite, den != 0)
        for (int ty = ty0; ty <= ty1; ++ty) {
            if (!owned_row(ty, bp.period, bp.mask)) continue;
            const int hrow = (LDSH ? owned_ord(bp, ty) : ty) * bp.tiles_x;
            for (int tx = tx0; tx <= tx1; ++tx) {
                if (LDSH) atomicAdd(&hist[hrow + tx], 1u);
                else atomicAdd(&tile_cnt[hrow + tx], 1u);
            }
        }
    }
    if (LDSH) {
        __syncthreads();
        for (int b = tid; b < hbins; b += 256) {
            const u32 h = hist[b];
            if (h) {
                const int r = b / bp.tiles_x;
                atomicAdd(&tile_cnt[owned_row_of(bp, r) * bp.tiles_x + (b - r * bp.tiles_x)], h);
            }
        }
    }
}

// Single workgroup: off[i] = sum(cnt[<i]) (off[ntiles] = P) and the work
// items of k_vis, {tile, list begin, list end, slices of the tile}: an owned
// tile has max(1, ceil(cnt/SLICE)) of them (an empty tile is one item: k_vis
// writes its pending clear); totals = {P, items, number of split tiles}.
// totals[3] = 1 when the pair list fits `cap` and the items `icap`; every later kernel of the
// batch reads it and does nothing otherwise (the host then re-runs the batch
// with an exact allocation before anything else is enqueued, nr_settle).
// It also re-zeroes the tile counters for the next batch (after reading them)
// and the emit cursors, and mirrors the totals into pinned host memory, so a
// batch needs no memset and no copy command.
// Work items of an owned tile with c pairs: one item when c <= lim (an empty
// tile too: k_vis writes its pending clears); a dense tile (c > lim) is split
// into ni = ceil(c / dsl) slices of equal length.  lim and dsl come from the
// batch's slice length (plan kernels: split_limits).
__device__ __forceinline__ u32 tile_items(u32 c, bool owned, u32 lim, u32 dsl) {
    if (!owned) return 0u;
    return c > lim ? (c + dsl - 1) / dsl : 1u;
}
// Work item k of the ni items of a tile with c pairs from list offset ea:
// {tile, slice begin, slice end, w}, w = ni (items sharing the tile's merge,
// low 16 bits) | k << 16.  Slices are ceil(c / ni) long (the last one shorter,
// never empty: ceil(c / ni) <= dsl).
__device__ __forceinline__ uint4 tile_item(u32 tile, u32 ea, u32 c, u32 k, u32 ni) {
    if (ni == 1) return make_uint4(tile, ea, ea + c, 1u);
    const u32 q = (c + ni - 1) / ni;
    const u32 ls = ea + k * q;
    return make_uint4(tile, ls, min(ls + q, ea + c), ni | (k << 16));
}
// Split limits of a batch from its slice length: a tile of more than lim =
// min(slice, split_at) pairs is split into slices of about dsl = min(lim,
// dslice) (>= SLICE_MIN) pairs.  Splitting only the dense tiles, finer than the
// whole-tile limit, shortens the longest work items (k_vis's critical path)
// without splitting the many medium tiles.
__device__ __forceinline__ void split_limits(u32 slice, u32 split_at, u32 dslice, u32& lim, u32& dsl) {
    lim = min(slice, split_at);
    dsl = max((u32)SLICE_MIN, min(lim, dslice));
}

constexpr int PLAN_W = PLAN_T / 64;
// Size classes of a tile's work items: 0 empty; 1..PLAN_ONE one slice, by
// the count's bin (below); the PLAN_SPLIT highest for tiles split over
// several slices, by their slice count (>= 8, 4-7, 2-3).  Items are laid out
// largest class first: k_vis workgroups take items in index order, so the
// long ones start first and the short ones fill the tail (a longest-first
// schedule).  Results do not depend on the order (order-free raster).  The
// split classes come first, so split items take the indices [0, slices) --
// their key slots.  The densest tiles' slices first (round 4): their last
// slice merges the others' keys and shades the tile, the kernel's longest
// chain (a 16-slice 1080p tile started 62 us into a 98 us raster,
// tools/exp/probe_items.py).
// One-slice classes are PLAN_ONE equal bins of [1, lim] (octaves had left a
// C3 frame's items -- nearly all in [256, 1024] -- in two classes, in tile
// order within each): C3 -0.8 %, 1M tris at 1080p -1.3 %,
// C2 -2 % per frame (profiles/r03_c3/ab_class_lin.txt).
constexpr int PLAN_ONE = 10, PLAN_SPLIT = 3, PLAN_NB = 1 + PLAN_ONE + PLAN_SPLIT;
// top: the upper end of the one-slice bins -- lim for a binning's plan, the
// largest one-slice count for the visible plan (k_vis_plan)
__device__ __forceinline__ int size_class(u32 c, u32 lim, u32 dsl, u32 top) {
    if (c > lim) {
        const u32 ni = (c + dsl - 1) / dsl;
        return PLAN_NB - (ni >= 8 ? 1 : ni >= 4 ? 2 : 3);
    }
    if (c == 0) return 0;
    return 1 + min((int)((float)c * ((float)PLAN_ONE / (float)(top + 1))), PLAN_ONE - 1);
}
__device__ __forceinline__ int size_class(u32 c, u32 lim, u32 dsl) { return size_class(c, lim, dsl, lim); }

// Tiles are taken PLAN_T at a time (thread = tile: coalesced), each round a
// workgroup scan carried over from the previous one.
__global__ __launch_bounds__(PLAN_T) void k_free_plan(u32* __restrict__ cnt, int ntiles, int tiles_x, int period,
                                                      u64 mask, u32* __restrict__ off, uint4* __restrict__ items,
                                                      u32* __restrict__ cur, u32* __restrict__ totals,
                                                      u64* __restrict__ host_totals, u32 cap, u32 icap, u32 seq,
                                                      u32 slice_target, u32 kcap, u32 split_at, u32 dslice) {
    __shared__ u32 sh[3][PLAN_W];
    __shared__ u32 bcnt[PLAN_NB], bcur[PLAN_NB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < PLAN_NB) bcnt[tid] = 0;
    // pass 0: the pair total sets the slice length, the smallest power of two
    // in [SLICE_MIN, SLICE] giving at most ~slice_target items of work
    // (short lists are sliced finer so that a sharded frame, whose dense tiles
    // are few, still fills the chip)
    u32 a = 0, hv = 0;
    for (int i = tid; i < ntiles; i += PLAN_T) {
        const u32 c = cnt[i];
        a += c;
        hv += c >= HEAVY_PAIRS ? 1u : 0u;
    }
    a = wave_scan(a, lane); hv = wave_scan(hv, lane);
    if (lane == 63) { sh[0][w] = a; sh[1][w] = hv; }
    __syncthreads();
    u32 ta = 0, th = 0;
#pragma unroll
    for (int k = 0; k < PLAN_W; ++k) { ta += sh[0][k]; th += sh[1][k]; }
    u32 slice = SLICE_MIN;
    while (slice < SLICE && (u64)slice * slice_target < ta) slice <<= 1;
    u32 lim, dsl;
    split_limits(slice, split_at, dslice, lim, dsl);
    __syncthreads();
    // pass 1: items (the capacity check needs the totals before any item is
    // written) and the number of items per size class
    u32 b = 0, m = 0;
    for (int i = tid; i < ntiles; i += PLAN_T) {
        const u32 c = cnt[i];
        const u32 ni = tile_items(c, owned_row(i / tiles_x, period, mask), lim, dsl);
        b += ni;
        m += ni > 1 ? ni : 0u;
        if (ni) atomicAdd(&bcnt[size_class(c, lim, dsl)], ni);
    }
    b = wave_scan(b, lane); m = wave_scan(m, lane);
    if (lane == 63) { sh[1][w] = b; sh[2][w] = m; }
    __syncthreads();
    u32 tb = 0, tm = 0;
#pragma unroll
    for (int k = 0; k < PLAN_W; ++k) { tb += sh[1][k]; tm += sh[2][k]; }
    const bool fits = ta <= cap && tb <= icap && tm <= kcap;
    if (tid == 0) {   // item ranges of the classes, largest class first
        u32 base = 0;
        for (int k = PLAN_NB - 1; k >= 0; --k) { bcur[k] = base; base += bcnt[k]; }
    }
    __syncthreads();
    // pass 2: offsets and items
    u32 carryA = 0;
    for (int r0 = 0; r0 < ntiles; r0 += PLAN_T) {
        const int i = r0 + tid;
        u32 c = 0, ni = 0;
        if (i < ntiles) {
            c = cnt[i];
            ni = tile_items(c, owned_row(i / tiles_x, period, mask), lim, dsl);
        }
        const u32 ia = wave_scan(c, lane);
        if (lane == 63) sh[0][w] = ia;
        __syncthreads();
        u32 ea = carryA + ia - c;
#pragma unroll
        for (int k = 0; k < PLAN_W; ++k) {
            if (k < w) ea += sh[0][k];
            carryA += sh[0][k];
        }
        __syncthreads();
        if (i < ntiles) {
            off[i] = ea;
            if (fits && ni) {
                const u32 eb = atomicAdd(&bcur[size_class(c, lim, dsl)], ni);
                for (u32 k = 0; k < ni; ++k) items[eb + k] = tile_item((u32)i, ea, c, k, ni);
            }
            cnt[i] = 0;
            cur[i] = 0;
        }
    }
    if (tid == 0) {
        off[ntiles] = ta;
        u32 t[PW_COUNT];
        t[PW_PAIRS] = ta; t[PW_ITEMS] = tb; t[PW_SPLIT] = tm; t[PW_FITS] = fits ? 1u : 0u;
        t[PW_SEQ] = seq; t[PW_HEAVY] = th; t[PW_LONGEST] = 0u;
        for (int k = 0; k < PW_DEV; ++k) totals[k] = t[k];
        // the host copy (nr_settle polls it): every word carries the batch's
        // sequence number in its high half and is stored on its own (8-byte
        // stores are single-copy atomic), so the host needs no ordering between
        // them and the kernel no release -- a system-scope release writes back
        // the whole L2 (buffer_wbl2), the dirty frame lines of the raster
        // running beside this kernel included (C3 -1.2 %, 8-way share -2 %,
        // profiles/r03_c3/ab_plan_release.txt)
        for (int k = 0; k < PW_COUNT; ++k)
            __hip_atomic_store(&host_totals[k], ((u64)seq << 32) | t[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The same plan with every tile count read once, into registers: thread t
// owns PR = 4 * ceil(ntiles / 4T) <= 16 consecutive tiles [t*PR, t*PR + PR), read and
// written as 16-byte vectors (the tile arrays are allocated to TILE_ARR entries,
// so the padding past ntiles -- never counted, so zero -- is in bounds), so
// the kernel makes one round of global loads instead of one per pass and per
// block of tiles.  Items are placed by size class without same-address LDS
// atomics (a wave's lanes mostly share a class, and such atomics serialise):
// per-lane class counts in registers, per-class wave scans, one LDS slot per
// (class, wave).  Launched with T = PLAN_T = 1024 threads whenever ntiles <=
// 16 * T (16384 tiles, an 8K frame; free_enqueue).
template <int T, int PR>
__global__ __launch_bounds__(T) void k_free_plan_r(u32* __restrict__ cnt, int ntiles, int tiles_x, int period,
                                                   u64 mask, u32* __restrict__ off, uint4* __restrict__ items,
                                                   u32* __restrict__ cur, u32* __restrict__ totals,
                                                   u64* __restrict__ host_totals, u32 cap, u32 icap, u32 seq,
                                                   u32 slice_target, u32 kcap, u32 split_at, u32 dslice, u32 maxc) {
    constexpr int NWV = T / 64;
    __shared__ u32 sh[4][NWV];
    __shared__ u32 smax;   // longest tile list (ordered batches sort each list in LDS: <= maxc, 0 = no limit)
    __shared__ u32 csh[PLAN_NB][NWV];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (((ntiles + T - 1) / T) + 3) & ~3;
    const int i0 = tid * per;
    u32 c[PR];
#pragma unroll
    for (int q = 0; q < PR / 4; ++q) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (4 * q < per) v = reinterpret_cast<const uint4*>(cnt + i0)[q];
        c[4 * q] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
    }
    u32 a = 0, hv = 0, mx = 0;
#pragma unroll
    for (int j = 0; j < PR; ++j) {
        a += c[j];
        hv += c[j] >= HEAVY_PAIRS ? 1u : 0u;
        mx = c[j] > mx ? c[j] : mx;
    }
    if (tid == 0) smax = 0;
    __syncthreads();
    if (maxc) atomicMax(&smax, mx);
    const u32 ia = wave_scan(a, lane), ih = wave_scan(hv, lane);
    if (lane == 63) { sh[0][w] = ia; sh[1][w] = ih; }
    __syncthreads();
    u32 ta = 0, th = 0, ea = ia - a;   // ea: list offset of this thread's first tile
#pragma unroll
    for (int k = 0; k < NWV; ++k) {
        if (k < w) ea += sh[0][k];
        ta += sh[0][k];
        th += sh[1][k];
    }
    u32 slice = SLICE_MIN;
    while (slice < SLICE && (u64)slice * slice_target < ta) slice <<= 1;
    u32 lim, dsl;
    split_limits(slice, split_at, dslice, lim, dsl);
    // items per tile, per-lane totals per size class (ownership: tile row of i0 + j)
    const int ty0 = i0 / tiles_x, tx0 = i0 - ty0 * tiles_x;
    u32 b = 0, m = 0, hc[PLAN_NB];
#pragma unroll
    for (int k = 0; k < PLAN_NB; ++k) hc[k] = 0;
    {
        int ty = ty0, tx = tx0;
#pragma unroll
        for (int j = 0; j < PR; ++j) {
            const u32 ni = (j < per && i0 + j < ntiles) ? tile_items(c[j], owned_row(ty, period, mask), lim, dsl) : 0u;
            b += ni;
            m += ni > 1 ? ni : 0u;
            const int cls = size_class(c[j], lim, dsl);
#pragma unroll
            for (int k = 0; k < PLAN_NB; ++k) hc[k] += cls == k ? ni : 0u;
            if (++tx == tiles_x) { tx = 0; ++ty; }
        }
    }
    // per class: this lane's exclusive position among the wave's items
#pragma unroll
    for (int k = 0; k < PLAN_NB; ++k) {
        const u32 inc = wave_scan(hc[k], lane);
        if (lane == 63) csh[k][w] = inc;
        hc[k] = inc - hc[k];
    }
    const u32 ib = wave_scan(b, lane), im = wave_scan(m, lane);
    if (lane == 63) { sh[2][w] = ib; sh[3][w] = im; }
    __syncthreads();
    u32 tb = 0, tm = 0;
#pragma unroll
    for (int k = 0; k < NWV; ++k) { tb += sh[2][k]; tm += sh[3][k]; }
    const bool fits = ta <= cap && tb <= icap && tm <= kcap && (!maxc || smax <= maxc);
    // class ranges, largest class first, and each wave's base inside them:
    // thread k < PLAN_NB turns column k of csh into the wave bases of class k.
    // Every column is read (into registers) before any is rewritten: thread k
    // sums the columns of the classes above k while their threads rewrite them.
    u32 start = 0, col[NWV];
    if (tid < PLAN_NB) {
        for (int k = PLAN_NB - 1; k > tid; --k)
            for (int q = 0; q < NWV; ++q) start += csh[k][q];
#pragma unroll
        for (int q = 0; q < NWV; ++q) col[q] = csh[tid][q];
    }
    __syncthreads();
    if (tid < PLAN_NB) {
#pragma unroll
        for (int q = 0; q < NWV; ++q) {
            csh[tid][q] = start;
            start += col[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PLAN_NB; ++k) hc[k] += csh[k][w];
    {   // c[j] becomes tile j's list offset
        int ty = ty0, tx = tx0;
#pragma unroll
        for (int j = 0; j < PR; ++j) {
            const u32 cj = c[j];
            c[j] = ea;
            const int i = i0 + j;
            const u32 ni = (j < per && i < ntiles) ? tile_items(cj, owned_row(ty, period, mask), lim, dsl) : 0u;
            const int cls = size_class(cj, lim, dsl);
            u32 eb = 0;
#pragma unroll
            for (int k = 0; k < PLAN_NB; ++k)
                if (cls == k) { eb = hc[k]; hc[k] += ni; }
            if (fits)
                for (u32 k = 0; k < ni; ++k) items[eb + k] = tile_item((u32)i, ea, cj, k, ni);
            ea += cj;
            if (++tx == tiles_x) { tx = 0; ++ty; }
        }
    }
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int q = 0; q < PR / 4; ++q) {
        if (4 * q < per) {
            reinterpret_cast<uint4*>(off + i0)[q] = make_uint4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
            reinterpret_cast<uint4*>(cnt + i0)[q] = z4;
            reinterpret_cast<uint4*>(cur + i0)[q] = z4;
        }
    }
    if (tid == 0) {
        off[ntiles] = ta;   // (the same value as the padding stores write there)
        u32 t[PW_COUNT];
        t[PW_PAIRS] = ta; t[PW_ITEMS] = tb; t[PW_SPLIT] = tm; t[PW_FITS] = fits ? 1u : 0u;
        t[PW_SEQ] = seq; t[PW_HEAVY] = th; t[PW_LONGEST] = smax;
        for (int k = 0; k < PW_DEV; ++k) totals[k] = t[k];
        for (int k = 0; k < PW_COUNT; ++k)   // (host copy: see k_free_plan)
            __hip_atomic_store(&host_totals[k], ((u64)seq << 32) | t[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <bool LDSH>
__global__ __launch_bounds__(256) void k_free_emit(const BinParams bp, const u32* __restrict__ off,
                                                   u32* __restrict__ cur, u32* __restrict__ list, int ntiles,
                                                   const u64* __restrict__ rects, const u32* __restrict__ plan) {
    extern __shared__ u32 hist[];
    if (!plan[PW_FITS]) return;
    const int tid = threadIdx.x;
    const i64 base = (i64)blockIdx.x * 256 * TPT;
    u64 rk[TPT];   // every rectangle first: one round of load latency
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        rk[k] = t < bp.src.n ? rects[t] : NO_RECT;
    }
    const int hbins = bp.hrows * bp.tiles_x;   // (owned tile rows only, as k_free_count)
    if (LDSH) {
        for (int b = tid; b < hbins; b += 256) hist[b] = 0;
        __syncthreads();
        for (int k = 0; k < TPT; ++k) {
            const i64 t = base + k * 256 + tid;
            if (t >= bp.src.n) break;
            const u64 rc = rk[k];
            if (rc == NO_RECT) continue;
            const int tx0 = (int)(rc & 0xFFFF), tx1 = (int)((rc >> 16) & 0xFFFF);
            const int ty0 = (int)((rc >> 32) & 0xFFFF), ty1 = (int)(rc >> 48);
            for (int ty = ty0; ty <= ty1; ++ty)
                if (owned_row(ty, bp.period, bp.mask)) {
                    const int hrow = owned_ord(bp, ty) * bp.tiles_x;
                    for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&hist[hrow + tx], 1u);
                }
        }
        __syncthreads();
        // reserve each touched tile's range once: hist[b] becomes the next slot
        for (int b = tid; b < hbins; b += 256) {
            const u32 h = hist[b];
            if (h) {
                const int r = b / bp.tiles_x;
                const int tile = owned_row_of(bp, r) * bp.tiles_x + (b - r * bp.tiles_x);
                hist[b] = off[tile] + atomicAdd(&cur[tile], h);
            }
        }
        __syncthreads();
    }
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        if (t >= bp.src.n) break;
        const u64 rc = rk[k];
        if (rc == NO_RECT) continue;
        const int tx0 = (int)(rc & 0xFFFF), tx1 = (int)((rc >> 16) & 0xFFFF);
        const int ty0 = (int)((rc >> 32) & 0xFFFF), ty1 = (int)(rc >> 48);
        for (int ty = ty0; ty <= ty1; ++ty) {
            if (!owned_row(ty, bp.period, bp.mask)) continue;
            const int hrow = (LDSH ? owned_ord(bp, ty) : ty) * bp.tiles_x;
            for (int tx = tx0; tx <= tx1; ++tx) {
                const u32 slot = LDSH ? atomicAdd(&hist[hrow + tx], 1u)
                                      : off[hrow + tx] + atomicAdd(&cur[hrow + tx], 1u);
                list[slot] = (u32)t;
            }
        }
    }
}

// Loose ranges (a moving scene): a tile of c pairs under the schedule's
// transform gets room for loose_cap(c) under a transform that moves no vertex
// more than LOOSE_PX (a quarter more, and 64 pairs for the triangles that move
// in across its edges).  k_loose_off: one workgroup, off2 = exclusive scan of
// loose_cap(off[t + 1] - off[t]), once per schedule.
__host__ __device__ __forceinline__ u32 loose_cap(u32 c) { return c + c / 4 + 64; }
__global__ __launch_bounds__(1024) void k_loose_off(const u32* __restrict__ off, u32* __restrict__ off2, int ntiles) {
    __shared__ u32 wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (ntiles + 1023) / 1024;
    const int t0 = tid * per, t1 = min(ntiles, t0 + per);
    u32 s = 0;
    for (int t = t0; t < t1; ++t) s += loose_cap(off[t + 1] - off[t]);
    const u32 inc = wave_scan(s, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    u32 run = inc - s;
    for (int k = 0; k < w; ++k) run += wsum[k];
    for (int t = t0; t < t1; ++t) {
        off2[t] = run;
        run += loose_cap(off[t + 1] - off[t]);
    }
    if (t0 < t1 && t1 == ntiles) off2[ntiles] = run;   // (the last non-empty chunk)
    if (ntiles == 0 && tid == 0) off2[0] = 0;
}

// Warm binning: a TriangleBuffer drawn again under the binning key of its
// last validated binning, whose tile offsets and work items the context keeps
// (TriScratch::Schedule).  One pass over the triangles -- screen rectangle
// (as k_free_count), the workgroup's LDS histogram of its pairs over the owned
// tile rows, one range reservation per touched tile, the pairs (as
// k_free_emit) -- into the same [off[t], off[t + 1]) ranges: the count pass,
// the plan and the host's validation of the cold path are not needed,
// because the same buffer under the same key gives every tile exactly its
// former count.  LDSH: hist (next slot) and hlim (range end) per owned tile in
// LDS.
// The set's pair cursors are not reset between warm batches: the epoch-th
// warm batch of one schedule on this set finds cur[t] = epoch * count(t) and
// takes slots from there (cursor - epoch * count, count = off[t + 1] - off[t]).
// Checks: a tile found over its range stores the batch's tag in
// wstat[WS_TAG] (beside the cursors; its excess pairs are dropped), and k_vis
// checks every tile's cursor before it trusts the tile's list: after the e-th
// warm batch cur[t] must be (e + 1) * count(t), so an undercount or an
// overcount of that tile is seen there, and only that tile falls back
// (WarmCheck; round 6 -- until round 5 every binning workgroup added its pair
// total to one global sum word: ~4000 atomics on one address, 3.5 us of the
// 1080p frame, profiles/r05/ab_pair_sum.txt).  `inject` (tests only,
// SetWarmFaultInjection): 1 shifts the epoch (every touched tile out of its
// range), 3 drops workgroup 0's pairs (an undercount of its tiles).
template <bool LDSH>
__global__ __launch_bounds__(256) void k_bin_warm(const BinParams bp, const u32* __restrict__ off,
                                                  u32* __restrict__ cur, u32* __restrict__ list,
                                                  u32* __restrict__ wstat, u32 tag, u32 epoch,
                                                  const f64* __restrict__ cbox, const u32* __restrict__ blocks,
                                                  u32 inject, u32 loose) {
    extern __shared__ u32 hist[];
    const int tid = threadIdx.x;
    // (fault 1 under loose ranges: every touched tile's count runs far past its range)
    const u32 over = loose && inject == 1 ? 0x100000u : 0u;
    if (inject == 1 && !loose) epoch += 7;
    if (inject == 3 && blockIdx.x == 0) return;
    // (blocks: the schedule's active blocks, warm_blocks; the others hold no
    // cluster that reaches an owned tile)
    const i64 base = (i64)(blocks ? blocks[blockIdx.x] : blockIdx.x) * 256 * TPT;
    const int hbins = bp.hrows * bp.tiles_x;
    u32* hlim = hist + hbins;
    // this wave's cluster of each of its TPT triangle groups (NR_CLUSTER == 64:
    // one wave, so the test and the skip are wave-uniform)
    static_assert(NR_CLUSTER == 64, "a cluster is one wave's triangles");
    bool cl[TPT];
    bool anyc = false;
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 c = (base + k * 256) / NR_CLUSTER + __builtin_amdgcn_readfirstlane(tid >> 6);
        cl[k] = !cbox || c * NR_CLUSTER >= bp.src.n || cluster_may_touch(bp, cbox + c * 4, CLUSTER_DEV);
        anyc = anyc || cl[k];
    }
    // a workgroup none of whose clusters reaches an owned tile has nothing to do
    // (most of them on a sharded frame's rank)
    if (cbox && !__syncthreads_or(anyc ? 1 : 0)) return;
    // (loading the positions before the cluster test -- one latency round
    // less, all bytes -- was not faster, round 4)
    f64 pxy[TPT][6];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        if (cl[k] && t < bp.src.n) load_tri_xy(bp.src.xy, t, pxy[k]);
    }
    if (LDSH) for (int b = tid; b < hbins; b += 256) hist[b] = 0;
    if (LDSH) __syncthreads();   // (hist zeroed)
    u64 rk[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        rk[k] = NO_RECT;
        if (t >= bp.src.n || !cl[k]) continue;
        f64 sx[3], sy[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) nr_xform(bp.m, pxy[k][2 * v], pxy[k][2 * v + 1], sx[v], sy[v]);
        int tx0, tx1, ty0, ty1;
        if (!tri_tiles(sx, sy, bp.W, bp.H, tx0, tx1, ty0, ty1)) continue;
        rk[k] = pack_rect(tx0, tx1, ty0, ty1);
        for (int ty = ty0; ty <= ty1; ++ty) {
            if (!owned_row(ty, bp.period, bp.mask)) continue;
            if (!LDSH) continue;
            const int hrow = owned_ord(bp, ty) * bp.tiles_x;
            for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&hist[hrow + tx], 1u);
        }
    }
    if (LDSH) {
        __syncthreads();
        for (int b = tid; b < hbins; b += 256) {   // reserve each touched tile's range once
            const u32 h = hist[b];
            if (h) {
                const int r = b / bp.tiles_x;
                const int tile = owned_row_of(bp, r) * bp.tiles_x + (b - r * bp.tiles_x);
                const u32 beg = off[tile], end = off[tile + 1];
                const u32 start = beg + atomicAdd(&cur[tile], h + over) - epoch * (end - beg);
                const bool bad = start < beg || start + h > end;
                hist[b] = bad ? end : start;   // (bad: every slot of this range fails slot < end)
                hlim[b] = end;
                // (loose ranges: an overflowing tile's cursor ends past its range, and k_vis
                // runs that tile over every triangle; the batch's other tiles are exact)
                if (bad && !loose) __hip_atomic_store(&wstat[WS_TAG], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (LDSH) __syncthreads();   // (LDS ranges reserved)
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const i64 t = base + k * 256 + tid;
        const u64 rc = rk[k];
        if (t >= bp.src.n || rc == NO_RECT) continue;
        const int tx0 = (int)(rc & 0xFFFF), tx1 = (int)((rc >> 16) & 0xFFFF);
        const int ty0 = (int)((rc >> 32) & 0xFFFF), ty1 = (int)(rc >> 48);
        for (int ty = ty0; ty <= ty1; ++ty) {
            if (!owned_row(ty, bp.period, bp.mask)) continue;
            const int hrow = (LDSH ? owned_ord(bp, ty) : ty) * bp.tiles_x;
            for (int tx = tx0; tx <= tx1; ++tx) {
                u32 slot, end;
                if (LDSH) {
                    slot = atomicAdd(&hist[hrow + tx], 1u);
                    end = hlim[hrow + tx];
                } else {
                    const u32 beg = off[hrow + tx];
                    end = off[hrow + tx + 1];
                    slot = beg + atomicAdd(&cur[hrow + tx], 1u + over) - epoch * (end - beg);
                    if (slot < beg || slot >= end) {
                        if (!loose) __hip_atomic_store(&wstat[WS_TAG], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        slot = end;
                    }
                }
                if (slot < end) list[slot] = (u32)t;
            }
        }
    }
}

// Same-queue hand-off from a warm binning beside the raster to the raster
// (NR_GATE, default on): the binning stream ends the batch's binning with
// k_gate_signal storing the set's next token, and the main stream runs
// k_gate_wait -- one thread polling the token -- right before the raster, in
// place of a cross-queue event wait, whose wake-up cost ~10 us per frame
// after a binning that had long finished (8-way share kernel trace,
// profiles/r04/ab_any_order.txt).  The binning kernel's completion (kernel
// boundary on the binning stream) makes its pairs visible before the token is
// stored.  k_gate_wait also hands the raster its plan words (a copy of the
// schedule's); should the token not arrive within a second, the copy says
// "did not fit" (the raster does nothing) and the host latches an error --
// no wave polls forever, no raster reads a half-written list.  The binning is
// enqueued before the wait on the host, so even two streams sharing one
// hardware queue cannot deadlock.  (A timed-out raster runs its fallback and
// reports, WarmCheck.)
__global__ void k_gate_signal(u32* __restrict__ gate, u32 tok) {
    if (threadIdx.x == 0) __hip_atomic_store(gate, tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Testing (SetWarmFaultInjection 4): holds the binning stream for 1.5 s before
// a warm binning, so that the raster's token wait (1 s) gives up first and the
// binning lands after the raster's fallback (one thread, bounded).
__global__ void k_delay_binning() {
    if (threadIdx.x != 0) return;
    const u64 t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
    while (__builtin_amdgcn_s_memrealtime() - t0 < 150000000ull) __builtin_amdgcn_s_sleep(127);
}
__global__ void k_gate_wait(const u32* __restrict__ gate, u32 tok, const u32* __restrict__ splan,
                            u32* __restrict__ gplan) {
    if (threadIdx.x != 0) return;
    const u64 t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
    bool ok = true;
    while (__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != tok) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull) {
            ok = false;
            break;
        }
    }
    for (int k = 0; k < PW_DEV; ++k) gplan[k] = (k == PW_FITS && !ok) ? 0u : splan[k];
}

// One workgroup per work item; the first item of each tile (slice 0) prunes
// the tile's pairs [off[t], off[t + 1]): those whose triangle is marked go, in
// their order, to vlist from off[t], and their number to vcnt[t].  A split tile
// (nsl slices) keeps at least nsl pairs -- k_vis cuts the count into nsl
// slices and none may be empty (its chunk length divides) -- padded with the
// tile's first unmarked pairs: a triangle more never changes the frame.  A
// split tile holds more pairs than slices, so the padding is always there.
__global__ __launch_bounds__(256) void k_prune_list(const uint4* __restrict__ items, const u32* __restrict__ off,
                                                    const u32* __restrict__ list, const u32* __restrict__ mask, u32 n,
                                                    u32* __restrict__ vlist, u32* __restrict__ vcnt,
                                                    u32* __restrict__ total) {
    __shared__ u32 wsum[4];
    const uint4 d = items[blockIdx.x];
    if (d.w >> 16) return;
    const u32 tile = d.x, nsl = d.w & 0xFFFFu;
    const u32 beg = off[tile], end = off[tile + 1];
    if (beg == end) return;   // (vcnt is zeroed before the launch)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    auto marked = [&](u32 t) -> u32 { return t < n ? (mask[t >> 5] >> (t & 31u)) & 1u : 0u; };
    u32 pad = 0;   // unmarked pairs a split tile keeps
    if (nsl > 1) {
        u32 m = 0;
        for (u32 i = beg + tid; i < end; i += 256) m += marked(list[i]);
        m = wave_scan(m, lane);
        if (lane == 63) wsum[w] = m;
        __syncthreads();
        const u32 tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
        pad = tot < nsl ? nsl - tot : 0u;
    }
    // a pair's place among the kept ones: the marked pairs before it + the
    // padding pairs before it (the first `pad` unmarked ones); marked and
    // unmarked counts of a 256-pair round are scanned together, 16 bits each
    u32 km = 0, ku = 0;   // marked / unmarked pairs of the rounds so far
    for (u32 b = beg; b < end; b += 256) {
        const u32 i = b + tid;
        const bool in = i < end;
        const u32 t = in ? list[i] : 0u;
        const u32 mk = in ? marked(t) : 0u;
        const u32 v = mk | ((in && !mk ? 1u : 0u) << 16);
        const u32 inc = wave_scan(v, lane);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        u32 ex = inc - v, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < w) ex += wsum[k];
            tot += wsum[k];
        }
        __syncthreads();
        const u32 ub = ku + (ex >> 16);
        if (in && (mk || ub < pad)) vlist[beg + km + (ex & 0xFFFFu) + min(ub, pad)] = t;
        km += tot & 0xFFFFu;
        ku += tot >> 16;
    }
    if (tid == 0) {
        const u32 c = km + min(ku, pad);
        vcnt[tile] = c;
        atomicAdd(total, c);
    }
}

// ---- visible plan -------------------------------------------------------------
// The pruned list sits at the full list's offsets, and the schedule's items
// are the full list's: a tile that held 3000 pairs is still split into three
// slices of ~150 kept pairs (each zeroes its keys, writes a 16 KB key slot and
// the last one merges them), and the items run longest first by the full
// counts.  k_vis_plan plans the kept counts afresh, once per pruning, on the
// main stream right after k_prune_list: a single workgroup, as k_free_plan,
// but it only reads the counts (they are the raster's cursors) and the offsets.
// Its items go to S.vitems and its totals to S.vplan; the layout is the plan
// kernels' (split tiles' items first -- item index = key slot -- the densest
// split tiles earliest, empty owned tiles last), so k_vis runs them unchanged:
// under the loose-format check it slices [off[t], off[t] + vcnt[t]) by the
// item's own slice count.
// One-slice classes: PLAN_ONE equal bins of [1, the largest one-slice count of
// this plan] -- bins of [1, lim] would leave the kept counts (C3: median 195
// of a limit of 1024) in two or three of the ten classes.
// Split limits: the visible plan's own (VIS_SPLIT_AT / VIS_DSLICE, or
// SetSplitLimits') under the schedule's slice length (lim_p, dsl_p: never
// coarser than the schedule's, and a small batch's short slices are kept).
// Finer limits than the schedule's can want more items or key
// slots than there are (icap, kcap: the real capacities): the kernel then
// plans under the schedule's limits (lim_s, dsl_s), under which no tile has
// more items than in the full plan, whose items and slots are allocated -- so
// the plan always fits and the host never waits or regrows for it.
// Measured (profiles/visible_replan/limits_table.md; ms per frame, parent ->
// limits 1024 / 512 / 256): C3 0.0769 -> 0.0700 / 0.0707 / 0.0698, 1M triangles
// at 1080p 0.0617 -> 0.0449 / 0.0513 / 0.0472, an 8-way C3 share 0.0271 ->
// 0.0218 / 0.0226 / 0.0217.  An item costs 20-35 us almost whatever its pairs
// (key set-up, shading), a slice that much again plus its slot, so the gain
// is the work no longer scheduled, and finer slices only add some back: the
// visible plan splits where the binning's plan does, at 1024.

__global__ __launch_bounds__(PLAN_T) void k_vis_plan(const u32* __restrict__ vcnt, const u32* __restrict__ off,
                                                     int ntiles, int tiles_x, int period, u64 mask,
                                                     uint4* __restrict__ items, u32* __restrict__ totals,
                                                     u64* __restrict__ host_totals, u32 icap, u32 kcap, u32 seq,
                                                     u32 lim_p, u32 dsl_p, u32 lim_s, u32 dsl_s) {
    __shared__ u32 sh[6][PLAN_W];
    __shared__ u32 smx[2];   // largest one-slice count under the preferred / the schedule's limits
    __shared__ u32 bcnt[PLAN_NB], bcur[PLAN_NB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < PLAN_NB) bcnt[tid] = 0;
    if (tid < 2) smx[tid] = 0;
    // pass 0: the kept total and the dense tiles
    u32 a = 0, hv = 0;
    for (int i = tid; i < ntiles; i += PLAN_T) {
        const u32 c = vcnt[i];
        a += c;
        hv += c >= HEAVY_PAIRS ? 1u : 0u;
    }
    a = wave_scan(a, lane); hv = wave_scan(hv, lane);
    if (lane == 63) { sh[0][w] = a; sh[1][w] = hv; }
    __syncthreads();
    u32 ta = 0, th = 0;
#pragma unroll
    for (int k = 0; k < PLAN_W; ++k) { ta += sh[0][k]; th += sh[1][k]; }
    u32 lim = lim_p, dsl = dsl_p;
    // pass 1: items and split slices under both pairs of limits
    u32 b = 0, m = 0, b2 = 0, m2 = 0, mx = 0, mx2 = 0;
    for (int i = tid; i < ntiles; i += PLAN_T) {
        const u32 c = vcnt[i];
        const bool owned = owned_row(i / tiles_x, period, mask);
        const u32 ni = tile_items(c, owned, lim, dsl), ni2 = tile_items(c, owned, lim_s, dsl_s);
        b += ni;
        m += ni > 1 ? ni : 0u;
        b2 += ni2;
        m2 += ni2 > 1 ? ni2 : 0u;
        if (owned && c <= lim) mx = max(mx, c);
        if (owned && c <= lim_s) mx2 = max(mx2, c);
    }
    b = wave_scan(b, lane); m = wave_scan(m, lane); b2 = wave_scan(b2, lane); m2 = wave_scan(m2, lane);
    if (lane == 63) { sh[2][w] = b; sh[3][w] = m; sh[4][w] = b2; sh[5][w] = m2; }
    if (mx) atomicMax(&smx[0], mx);
    if (mx2) atomicMax(&smx[1], mx2);
    __syncthreads();
    u32 tb = 0, tm = 0, tb2 = 0, tm2 = 0;
#pragma unroll
    for (int k = 0; k < PLAN_W; ++k) { tb += sh[2][k]; tm += sh[3][k]; tb2 += sh[4][k]; tm2 += sh[5][k]; }
    const bool pref = tb <= icap && tm <= kcap;
    if (!pref) { lim = lim_s; dsl = dsl_s; tb = tb2; tm = tm2; }
    const u32 top = max(smx[pref ? 0 : 1], 1u);
    const bool fits = tb <= icap && tm <= kcap;   // (always: see above)
    // pass 2: items per size class
    for (int i = tid; i < ntiles; i += PLAN_T) {
        const u32 c = vcnt[i];
        const u32 ni = tile_items(c, owned_row(i / tiles_x, period, mask), lim, dsl);
        if (ni) atomicAdd(&bcnt[size_class(c, lim, dsl, top)], ni);
    }
    __syncthreads();
    if (tid == 0) {   // item ranges of the classes, largest class first
        u32 base = 0;
        for (int k = PLAN_NB - 1; k >= 0; --k) { bcur[k] = base; base += bcnt[k]; }
    }
    __syncthreads();
    // pass 3: the items
    if (fits) {
        for (int i = tid; i < ntiles; i += PLAN_T) {
            const u32 c = vcnt[i];
            const u32 ni = tile_items(c, owned_row(i / tiles_x, period, mask), lim, dsl);
            if (!ni) continue;
            const u32 eb = atomicAdd(&bcur[size_class(c, lim, dsl, top)], ni), ea = off[i];
            for (u32 k = 0; k < ni; ++k) items[eb + k] = tile_item((u32)i, ea, c, k, ni);
        }
    }
    if (tid == 0) {
        u32 t[PW_COUNT];
        t[PW_PAIRS] = ta; t[PW_ITEMS] = tb; t[PW_SPLIT] = tm; t[PW_FITS] = fits ? 1u : 0u;
        t[PW_SEQ] = seq; t[PW_HEAVY] = th; t[PW_LONGEST] = 0u;
        for (int k = 0; k < PW_DEV; ++k) totals[k] = t[k];
        for (int k = 0; k < PW_COUNT; ++k)   // (host copy: see k_free_plan)
            __hip_atomic_store(&host_totals[k], ((u64)seq << 32) | t[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The key items of a pruned list (one workgroup, once per pruning, main stream
// right after k_prune_list): one item per owned tile {tile, slot, kept pairs, 0}
// -- the tiles with a kept pair first, densest first by KEY_NB equal bins of
// [1, the largest kept count], each one's slot its item index; then the owned
// tiles without one (slot ~0) -- no slices, whatever the split limits.
// ktile[t]: tile t's slot, ~0 when it has none (the capture frame's table).
// totals / host_totals (seq-tagged words, as the plan kernels'): {cached tiles, items}.
constexpr int KEY_NB = 16;
__global__ __launch_bounds__(PLAN_T) void k_key_plan(const u32* __restrict__ vcnt, int ntiles, int tiles_x, int period,
                                                     u64 mask, uint4* __restrict__ items, u32* __restrict__ ktile,
                                                     u32* __restrict__ totals, u64* __restrict__ host_totals, u32 seq) {
    __shared__ u32 bcnt[KEY_NB + 1], bcur[KEY_NB + 1];   // [0]: the empty owned tiles
    __shared__ u32 smx;
    const int tid = threadIdx.x;
    if (tid <= KEY_NB) bcnt[tid] = 0;
    if (tid == 0) smx = 0;
    __syncthreads();
    u32 mx = 0;
    for (int i = tid; i < ntiles; i += PLAN_T)
        if (owned_row(i / tiles_x, period, mask)) mx = max(mx, vcnt[i]);
    if (mx) atomicMax(&smx, mx);
    __syncthreads();
    const u32 top = smx;
    auto cls = [&](u32 c) -> int {
        return c == 0 ? 0 : 1 + min((int)((float)c * ((float)KEY_NB / (float)(top + 1))), KEY_NB - 1);
    };
    for (int i = tid; i < ntiles; i += PLAN_T)
        if (owned_row(i / tiles_x, period, mask)) atomicAdd(&bcnt[cls(vcnt[i])], 1u);
    __syncthreads();
    if (tid == 0) {   // densest class first, the empty tiles last
        u32 base = 0;
        for (int k = KEY_NB; k >= 0; --k) { bcur[k] = base; base += bcnt[k]; }
    }
    __syncthreads();
    for (int i = tid; i < ntiles; i += PLAN_T) {
        u32 slot = ~0u;
        if (owned_row(i / tiles_x, period, mask)) {
            const u32 c = vcnt[i];
            const u32 e = atomicAdd(&bcur[cls(c)], 1u);
            if (c) slot = e;
            items[e] = make_uint4((u32)i, slot, c, 0u);
        }
        ktile[i] = slot;
    }
    __syncthreads();
    if (tid == 0) {
        const u32 nit = bcur[0], nc = nit - bcnt[0];   // (bcur[0] has run to the end of the items)
        totals[0] = nc; totals[1] = nit;
        __hip_atomic_store(&host_totals[0], ((u64)seq << 32) | nc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host_totals[1], ((u64)seq << 32) | nit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// A kernel on stream s, its completion carried by `stop` when there is one.
// (Arguments are passed as they are typed here, unconverted: each launch
// function below takes exactly its kernel's parameter types.)
template <class K, class... A>
void enqueue(K kernel, dim3 grid, dim3 block, u32 lds, hipStream_t s, hipEvent_t stop, A... args) {
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, nullptr, stop, 0, args...);
}

// grid of the count and emit passes
int bin_blocks(const BinParams& bp) { return (int)((bp.src.n + 256 * TPT - 1) / (256 * TPT)); }

}  // namespace

// (LDS histograms: the owned tile rows)
void launch_free_count(const BinParams& bp, u32* tile_cnt, int ntiles, u64* rects, f64* rec, bool ordered, hipStream_t s,
                       hipEvent_t stop) {
    const int hbins = bp.hrows * bp.tiles_x;
    const bool ldsh = hbins <= LDS_HIST_MAX;
    const u32 hbytes = ldsh ? (u32)((size_t)hbins * sizeof(u32)) : 0u;
    const auto count = ordered ? (ldsh ? k_free_count<true, true> : k_free_count<false, true>)
                               : (ldsh ? k_free_count<true> : k_free_count<false>);
    enqueue(count, dim3(bin_blocks(bp)), dim3(256), hbytes, s, stop, bp, tile_cnt, ntiles, rects, rec);
}

void launch_free_plan(u32* cnt, int ntiles, int tiles_x, int period, u64 mask, u32* off, uint4* items, u32* cur,
                      u32* totals, u64* host_totals, u32 cap, u32 icap, u32 seq, u32 kcap, u32 split_at, u32 dslice,
                      u32 maxc, bool ordered, hipStream_t s, hipEvent_t stop) {
    if (ntiles <= PLAN_T * PR_MAX || ordered) {   // (ordered: ntiles <= ORD_BIN_TILES)
        // the register plan: one 1024-thread workgroup, PR = tiles per
        // thread -> 4, 8 or 16 (PR 4: 107 VGPRs; PR 8 and 16 spill a few,
        // 4 and 39, at __launch_bounds__(1024)'s 128).  It needs a whole CU
        // (an ordered batch's plan beside the ordered raster therefore waits
        // for the raster's tail, which measured better than a 512-thread
        // instance that runs the chain earlier, beside it: C5 +10 %,
        // profiles/r03_c5/ab_plan512.txt).  A 256-thread multi-round plan
        // that fits beside a running k_vis was kept for large batches until
        // round 5 (C3 0.163 vs 0.172 ms then, profiles/r02_c3/ab_plan_r.txt);
        // with the faster raster the chain's count ends with the raster and
        // the wide plan is faster: a cold C3 frame (c3_animated) 0.157 ->
        // 0.150 ms (profiles/r05/ab_plan_wide.txt).
        const int per = (ntiles + PLAN_T - 1) / PLAN_T;
#define NR_PLAN_R(PP) enqueue(k_free_plan_r<PLAN_T, PP>, dim3(1), dim3(PLAN_T), 0, s, stop, cnt, ntiles, tiles_x, period, \
                              mask, off, items, cur, totals, host_totals, cap, icap, seq, SLICE_TARGET, kcap, split_at, \
                              dslice, maxc)
        if (per <= 4) NR_PLAN_R(4); else if (per <= 8) NR_PLAN_R(8); else NR_PLAN_R(16);
#undef NR_PLAN_R
    }
    else
        enqueue(k_free_plan, dim3(1), dim3(1024), 0, s, stop, cnt, ntiles, tiles_x, period, mask, off, items, cur, totals,
                host_totals, cap, icap, seq, SLICE_TARGET, kcap, split_at, dslice);
}

void launch_free_emit(const BinParams& bp, const u32* off, u32* cur, u32* list, int ntiles, const u64* rects,
                      const u32* plan, hipStream_t s, hipEvent_t stop) {
    const int hbins = bp.hrows * bp.tiles_x;
    const bool ldsh = hbins <= LDS_HIST_MAX;
    const u32 hbytes = ldsh ? (u32)((size_t)hbins * sizeof(u32)) : 0u;
    enqueue(ldsh ? k_free_emit<true> : k_free_emit<false>, dim3(bin_blocks(bp)), dim3(256), hbytes, s, stop, bp, off, cur,
            list, ntiles, rects, plan);
}

void launch_loose_off(const u32* off, u32* off2, int ntiles, hipStream_t s, hipEvent_t stop) {
    enqueue(k_loose_off, dim3(1), dim3(1024), 0, s, stop, off, off2, ntiles);
}

// (LDSH: the next slot and the range end of every owned tile, 2 * hbins words)
void launch_bin_warm(const BinParams& bp, const u32* off, u32* cur, u32* list, u32* wstat, u32 tag, u32 epoch,
                     const f64* cbox, const u32* blocks, u32 inject, u32 loose, int grid, hipStream_t s, hipEvent_t stop) {
    const int hbins = bp.hrows * bp.tiles_x;
    const bool ldsh = 2 * hbins <= LDS_HIST_MAX;
    enqueue(ldsh ? k_bin_warm<true> : k_bin_warm<false>, dim3(grid), dim3(256), ldsh ? (u32)(2 * hbins * sizeof(u32)) : 0u,
            s, stop, bp, off, cur, list, wstat, tag, epoch, cbox, blocks, inject, loose);
}

void launch_gate_signal(u32* gate, u32 tok, hipStream_t s, hipEvent_t stop) {
    enqueue(k_gate_signal, dim3(1), dim3(64), 0, s, stop, gate, tok);
}
void launch_delay_binning(hipStream_t s, hipEvent_t stop) { enqueue(k_delay_binning, dim3(1), dim3(64), 0, s, stop); }
void launch_gate_wait(const u32* gate, u32 tok, const u32* splan, u32* gplan, hipStream_t s, hipEvent_t stop) {
    enqueue(k_gate_wait, dim3(1), dim3(64), 0, s, stop, gate, tok, splan, gplan);
}

// (one workgroup per work item of the schedule)
void launch_prune_list(const uint4* items, u32 nitems, const u32* off, const u32* list, const u32* mask, u32 n,
                       u32* vlist, u32* vcnt, u32* total, hipStream_t s, hipEvent_t stop) {
    enqueue(k_prune_list, dim3(nitems), dim3(256), 0, s, stop, items, off, list, mask, n, vlist, vcnt, total);
}

void launch_vis_plan(const u32* vcnt, const u32* off, int ntiles, int tiles_x, int period, u64 mask, uint4* items,
                     u32* totals, u64* host_totals, u32 icap, u32 kcap, u32 seq, u32 lim_p, u32 dsl_p, u32 lim_s,
                     u32 dsl_s, hipStream_t s, hipEvent_t stop) {
    enqueue(k_vis_plan, dim3(1), dim3(PLAN_T), 0, s, stop, vcnt, off, ntiles, tiles_x, period, mask, items, totals,
            host_totals, icap, kcap, seq, lim_p, dsl_p, lim_s, dsl_s);
}

void launch_key_plan(const u32* vcnt, int ntiles, int tiles_x, int period, u64 mask, uint4* items, u32* ktile,
                     u32* totals, u64* host_totals, u32 seq, hipStream_t s, hipEvent_t stop) {
    enqueue(k_key_plan, dim3(1), dim3(PLAN_T), 0, s, stop, vcnt, ntiles, tiles_x, period, mask, items, ktile, totals,
            host_totals, seq);
}

}  // namespace nrtri
