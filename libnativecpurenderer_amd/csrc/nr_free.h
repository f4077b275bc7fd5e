// nr_free.h — what the three files of the visibility-buffer raster share:
// nr_tri_free.hip (the host side of a batch), nr_free_bin.hip (the binning,
// planning and pruning kernels) and nr_free_vis.hip (the raster and shading
// kernels).  Kernels stay private to their file; the host reaches them through
// the launch functions declared at the end.  Internal to those three files:
// everything other files need is in nr_tri.h.
#pragma once
#include "nr_tri.h"

namespace nrtri {

constexpr int VWG = 256;  // k_vis workgroup
constexpr u32 SLICE = 1024;      // longest work item (triangles)
constexpr u32 SLICE_MIN = 64;    // shortest slice of a split tile
// Items the plan kernel aims for when it picks the slice length.  Round 4
// (warm binning, spill-free k_vis): 256, i.e. slices of 1024 for every batch of
// >= 2^17 owned pairs.  An 8-way C3 share (~150k pairs) used to get slices of
// 512: its split tiles' slot merges cost more than the longer slices (0.046 ->
// 0.041 ms per frame, C2 -1 %, C3 unchanged; profiles/r04/ab_slice_target.txt).
constexpr u32 SLICE_TARGET = 256;
constexpr int TPT = 4;   // triangles per thread in the binning kernels (2 / 8 measured slower, round 4)
constexpr int LDS_HIST_MAX = 16384;
constexpr int PLAN_T = 1024;       // the plan kernels' workgroup
constexpr u32 HEAVY_PAIRS = 256;   // a dense tile (for the k_vis workgroup-size choice)
constexpr int PR_MAX = 16;         // k_free_plan_r: tiles per thread, at most
constexpr int TILE_ARR = 16 * 1024 + 4;   // minimum length of the per-tile arrays
constexpr f64 COOP_PAIRS = 2.0;   // tile pairs per triangle above which k_vis takes the flattened raster
// Split limits of dense tiles (split_limits): a tile of more pairs than
// min(slice, SPLIT_AT) is split into slices of about DSLICE pairs (SetSplitLimits
// overrides them per context).
constexpr u32 SPLIT_AT = 1024, DSLICE = 1024;
constexpr u32 VIS_SPLIT_AT = 1024, VIS_DSLICE = 1024;   // the visible plan's own (k_vis_plan, nr_free_bin.hip)

// the warm checks' words, right after a set's ntiles cursors: WS_TAG the tag of
// a batch with a tile over its range, WS_REP the tag of the last batch whose
// failure a k_vis workgroup reported (one report per batch)
enum { WS_REP = 0, WS_TAG = 1 };

// Inclusive wave scan (64 lanes) with DPP row shifts and row broadcasts
// (VALU, a few cycles per step): Hillis-Steele inside each row of 16 lanes,
// then row 0's total into row 1 and row 2's into row 3 (row_bcast:15), then
// row 1's into rows 2 and 3 (row_bcast:31).  The __shfl_up form is a chain of
// six dependent LDS permutes (~100+ cycles each).
__device__ __forceinline__ u32 wave_scan(u32 v, int) {
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31
    return v;
}

// Can a cluster (user-space box {xmin, ymin, xmax, ymax}, TriangleBuffer::cbox)
// put a pair into an owned tile?  Its corners' screen positions bound every
// vertex's (the affine map's rounded products and sums are monotone in x and
// y), so a triangle's rows [ceil(ymin), ceil(ymax)) lie in the corners' row
// range (one row of margin each side); non-finite boxes are never culled.
// Columns follow tri_tiles: a triangle with a screen coordinate beyond 1e7
// is binned into every column of its rows, so a box with a corner beyond
// 1e7 (which may hold such a vertex) is never culled by x.
// The margins are the caller's: px columns and rows rows each side, and a box
// with a corner beyond hugeAt is not culled by x.  The device test takes
// CLUSTER_DEV; the host's list of a schedule's active binning blocks
// (warm_blocks) CLUSTER_HOST -- wider in every margin, so a superset.
struct ClusterMargins { f64 px, rows, hugeAt; };
constexpr ClusterMargins CLUSTER_DEV = {4.0, 1.0, 1e7}, CLUSTER_HOST = {12.0, 3.0, 5e6};
__host__ __device__ __forceinline__ bool cluster_may_touch(const BinParams& bp, const f64* box, const ClusterMargins mg) {
    f64 y0 = INFINITY, y1 = -INFINITY, x0 = INFINITY, x1 = -INFINITY;
    bool huge = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f64 sx, sy;
        nr_xform(bp.m, box[(c & 1) ? 2 : 0], box[(c & 2) ? 3 : 1], sx, sy);
        if (!std::isfinite(sx) || !std::isfinite(sy)) return true;
        huge = huge || fabs(sx) > mg.hugeAt || fabs(sy) > mg.hugeAt;
        y0 = fmin(y0, sy); y1 = fmax(y1, sy); x0 = fmin(x0, sx); x1 = fmax(x1, sx);
    }
    if (!huge && (x1 < -mg.px || x0 > (f64)bp.W + mg.px)) return false;
    const f64 r0 = fmax(ceil(y0) - mg.rows, 0.0), r1 = fmin(ceil(y1) + mg.rows, (f64)bp.H);
    if (!(r0 < r1)) return false;
    if (bp.period == 1) return true;
    const int ty0 = (int)r0 / TH, ty1 = ((int)r1 - 1) / TH;
    for (int ty = ty0; ty <= ty1 && ty < ty0 + 64; ++ty)
        if (owned_row(ty, bp.period, bp.mask)) return true;
    return ty1 >= ty0 + 64;
}

// The checks of a warm batch (k_bin_warm).  Batch-wide: the tag word
// wstat[WS_TAG] != this batch's tag (no tile over its range) and the plan says
// it fits (plan[PW_FITS] == 0: the binning's token never came, k_gate_wait);
// otherwise the raster runs its work items over EVERY triangle of the batch
// instead of the tile lists -- slow, but the same frame bit for bit (a
// triangle that misses a tile adds nothing to it).  Per tile: the tile's
// cursor == mult * its count (mult = epoch + 1: the cursors run on across a
// schedule's warm batches, k_bin_warm); otherwise only that tile's items run
// over every triangle.  The first workgroup to see a failure (wstat[WS_REP]
// exchanged for the batch's tag) reports it in host-mapped *hfail (reason 1 a
// tile over its range, 2 token timeout, 3 a tile's count wrong, 4 a tile over
// its loose range; nr_settle latches an error and drops the schedule, or for
// 4 stops binning that buffer loose).  wstat null: a cold batch (plan[PW_FITS] == 0
// there: the batch does nothing, the host re-runs it).
// Loose batches (a changed transform, loose ranges off = off2): the cursors
// start at 0 and hold the tile's pair count n, which only has to fit the
// tile's range; the tile's items then slice its n pairs afresh (item k of
// nsl: [k n / nsl, (k + 1) n / nsl)).
struct WarmCheck {
    u32* wstat;
    const u32* cur;   // the set's cursors
    const u32* off;   // the schedule's tile offsets (loose: its loose ranges)
    u32 tag, mult;
    u32* hfail;
    u32 loose;
};

// k_vis runs 2 * VWG-thread workgroups when the last batch had a few dense
// tiles (>= HEAVY_PAIRS pairs), fewer than WIDE_HEAVY (half the chip's k_vis
// workgroup slots): each dense item is then latency-bound at low occupancy
// and gains from more waves (C3 sharded 8 ways -18 %, 4 ways -14 %; 2 ways
// +6 %, hence the threshold); with many dense tiles (C3 unsharded, 2 ways)
// or none (C2) the narrow workgroups are faster.  (A 3-wave-per-SIMD
// instance, which left the next batch's binning a slot beside the raster, was
// dropped in round 5: 4 waves measured faster once k_vis was spill-free, C3
// 0.147 -> 0.140 ms, profiles/r04/ab_instances.txt.)
// Round 6 re-measure (profiles/r06/ab_wide_heavy.txt): with ~226 dense tiles (C3
// 8-way share) wide is 24 % faster; with ~444 (4-way share) and ~478 (1M
// triangles at 1080p) the narrow one is 7 % faster, so the threshold moved
// from 512 to 320.
constexpr u32 WIDE_HEAVY = 320;

// The key index of a key cache (k_key_index, once per generation, right after the capture frame): per cached
// slot s the dense number of every pixel's winner among the tile's staged winners, those winners' ids and their
// count -- a function of the slot's keys alone, so k_keys_idx (cached Gouraud batches) neither de-duplicates a
// tile's winners nor probes for a pixel's record.
constexpr int KI_RT = 280;                   // staged winners per tile (whatever the attribute mode)
constexpr unsigned short KI_NONE = 0xFFFF;   // the pixel has no winner ((u32)key == 0, or it lies past the frame edge)
constexpr unsigned short KI_DIRECT = 0xFFFE; // its winner is not staged: the record is loaded directly
struct KeyIndex {
    const unsigned short* idx = nullptr;   // [s][TH * TW], p = ly * TW + lx: the winner's dense number d (staged:
                                           // d < cnt[2 s]; else its record is loaded directly), or KI_NONE
    const u32* win = nullptr;              // [s][KI_RT]: the staged winners' ids (1-based, as the keys'), dense order
    const u32* cnt = nullptr;              // [s][2]: min(distinct winners, KI_RT), KI_DIRECT pixels
};
constexpr size_t KI_SLOT_BYTES = (size_t)TH * TW * 2 + (size_t)KI_RT * 4 + 8;   // of the index, per cached tile

// The key records of a key cache (k_key_records, once per generation, after the host has seen their total): the
// Gouraud shading record of every distinct winner of every cached slot, slot s's from record roff[s] in dense
// order -- a function of the buffer and the transform (part of the binning key) alone, so k_keys_rec copies a
// slot's staged records where k_keys_idx gathers their sources and builds them, and reads a record past KR_RT
// (below) by its pixel's dense number.  Sizes: nr_key_records.h.
struct KeyRecords {
    const f64* rec = nullptr;    // [roff[slots] + 1][16] (nr_key_records.h room_doubles)
    const u32* roff = nullptr;   // [slots + 1]
    u32 cached = 0, items = 0;   // the key plan's totals {cached tiles, items} as the host has seen them (kplan's words)
};
// k_keys_rec's own staging: the first KR_RT records of a slot are copied into LDS (the index's KI_RT is not
// involved: k_key_index writes true dense numbers and roff is uncapped, so a pixel whose number is KR_RT or more
// loads its record from the store).  248: 8 copy units per thread of a 256-thread workgroup exactly, and C3
// measured 1.5 % faster than at 280 (profiles/key_records/ab_experiments.txt (c), profiles/steady_rec).
constexpr int KR_RT = 248;
// The LDS stride of a staged record, in 16-byte units: a record's 8, and one of padding -- at 128 bytes every
// record starts on bank 0 or 32, at 144 sixteen consecutive records start on sixteen different banks.
constexpr int KR_LU = 9;
// Work units of a k_keys_rec launch: one per cached item, then one per run of (workgroup size / 64) empty items --
// the key plan puts the empty items last, and a wave clears one.
inline u32 keys_rec_units(u32 cached, u32 items, bool wide) {
    const u32 e = (u32)(wide ? 2 * VWG : VWG) / 64;
    return cached + (items - cached + e - 1) / e;
}

// The k_vis inputs of one batch: its work items, pair list and plan totals
// (a binning set's, or the warm schedule's).
struct VisArgs {
    const uint4* items;
    const u32* list;
    const u32* plan;
    WarmCheck wc;   // (a warm batch's checks; zero: a cold batch)
    // key cache (warm_enqueue): capture, the batch is the capture frame (its snapshot's kcap is set); kkeys
    // non-null, it is shaded from the cache by k_keys (kitems, kplan) and reads nothing of the above
    bool capture = false;
    const u64* kkeys = nullptr;
    const uint4* kitems = nullptr;
    const u32* kplan = nullptr;
    // key index (below): non-null, a cached Gouraud batch is shaded by k_keys_idx from the slots' winner index
    KeyIndex kindex;
    // key records (below): non-null, the k_keys_idx batch is shaded by k_keys_rec from the slots' records
    KeyRecords krec;
    // deferred stores (nr_common.h DeferredStores): the k_keys_idx / k_keys_rec batch writes the frame output alone
    bool defer = false;
};

// What a deferred batch's resolve runs over (TriScratch::DeferredStores::snap): the batch's snapshot by value --
// the buffer's arrays, the transform, the colour transform, the clear values -- the key fields of its VisArgs
// (kitems, kkeys, kplan, kindex), its grid and whether it ran the 512-thread instance.
struct DeferredSnapshot {
    FrameParams fp;
    VisArgs va{};
    u32 grid = 0;
    bool wide = false;
};

// ---- launch functions ---------------------------------------------------
// One per kernel: it picks the template instance and enqueues it on stream s;
// stop (optional) is carried by the kernel's own completion signal.  None
// checks hipGetLastError: the caller does, where it did.

// nr_free_bin.hip.  The count and emit grids cover bp.src.n triangles, 256 * TPT
// per workgroup; a warm binning's grid is the caller's (the schedule's active
// blocks, or as many).
void launch_free_count(const BinParams& bp, u32* tile_cnt, int ntiles, u64* rects, f64* rec, bool ordered, hipStream_t s,
                       hipEvent_t stop);
// (the register plan for up to PLAN_T * PR_MAX tiles and for every ordered batch; maxc: ordered batches only)
void launch_free_plan(u32* cnt, int ntiles, int tiles_x, int period, u64 mask, u32* off, uint4* items, u32* cur,
                      u32* totals, u64* host_totals, u32 cap, u32 icap, u32 seq, u32 kcap, u32 split_at, u32 dslice,
                      u32 maxc, bool ordered, hipStream_t s, hipEvent_t stop);
void launch_free_emit(const BinParams& bp, const u32* off, u32* cur, u32* list, int ntiles, const u64* rects,
                      const u32* plan, hipStream_t s, hipEvent_t stop);
void launch_loose_off(const u32* off, u32* off2, int ntiles, hipStream_t s, hipEvent_t stop);
void launch_bin_warm(const BinParams& bp, const u32* off, u32* cur, u32* list, u32* wstat, u32 tag, u32 epoch,
                     const f64* cbox, const u32* blocks, u32 inject, u32 loose, int grid, hipStream_t s, hipEvent_t stop);
void launch_gate_signal(u32* gate, u32 tok, hipStream_t s, hipEvent_t stop);
void launch_delay_binning(hipStream_t s, hipEvent_t stop);
void launch_gate_wait(const u32* gate, u32 tok, const u32* splan, u32* gplan, hipStream_t s, hipEvent_t stop);
void launch_prune_list(const uint4* items, u32 nitems, const u32* off, const u32* list, const u32* mask, u32 n,
                       u32* vlist, u32* vcnt, u32* total, hipStream_t s, hipEvent_t stop);
void launch_vis_plan(const u32* vcnt, const u32* off, int ntiles, int tiles_x, int period, u64 mask, uint4* items,
                     u32* totals, u64* host_totals, u32 icap, u32 kcap, u32 seq, u32 lim_p, u32 dsl_p, u32 lim_s,
                     u32 dsl_s, hipStream_t s, hipEvent_t stop);
void launch_key_plan(const u32* vcnt, int ntiles, int tiles_x, int period, u64 mask, uint4* items, u32* ktile,
                     u32* totals, u64* host_totals, u32 seq, hipStream_t s, hipEvent_t stop);

// nr_free_vis.hip
// the key index of `tiles` cached slots (one workgroup each) from their captured keys; W, H, tiles_x: the frame's
// (dist, when given: every slot's distinct winner count, uncapped)
void launch_key_index(const uint4* kitems, const u64* kkeys, u32 tiles, unsigned short* idx, u32* win, u32* cnt,
                      u32* dist, i64 W, i64 H, int tiles_x, hipStream_t s);
// the record offsets roff[tiles + 1] of the slots' distinct counts, and their total into host_total under seq
void launch_key_record_scan(const u32* dist, u32 tiles, u32* roff, u64* host_total, u32 seq, hipStream_t s);
// the records of `tiles` cached slots (one workgroup each) from their keys and index, under fp's buffer and transform
void launch_key_records(const FrameParams& fp, const u64* kkeys, u32 tiles, const unsigned short* idx, const u32* roff,
                        f64* rec, hipStream_t s);
// k_vis' ZMODE of a batch: 0 no test, 1 LESS + write, 2 LESS without write
int z_mode(const FrameParams& fp);
// k_vis (or, for a batch shaded from the key cache, k_keys / k_keys_idx) over `grid` workgroups
void launch_vis_any(const FrameParams& fp, const TriScratch& sc, const BatchTotals& t, const VisArgs& va, u32 grid,
                    hipStream_t s, hipEvent_t start, hipEvent_t stop);
// does a batch shaded from the key cache whose totals are t run the 512-thread instances?  (launch_vis' rule)
bool keys_wide(const BatchTotals& t);
// the pending f64 values (colour) and / or depths (depth; LESS + write batches only) of a deferred k_keys_idx
// batch: its snapshot, its key fields of va, its grid and workgroup size
void launch_keys_resolve(const FrameParams& fp, const VisArgs& va, u32 grid, bool wide, bool colour, bool depth,
                         hipStream_t s);

}  // namespace nrtri
