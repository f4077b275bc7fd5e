// nr_tri_free.hip — visibility-buffer raster for opaque batches.
//
// When every fragment of a batch overwrites (every vertex alpha == 1 and
// colourTransform[3] == 1, so ApplyPixel's `a != 1` blend never runs) the
// sequential semantics reduce, per pixel, to an order-independent reduction:
//   Z LESS + write : winner = min over (zq, tri) with zq < z_init -> min of
//                    the packed key (zq << 32) | (tri + 1), init z_init << 32
//   Z LESS, no write: winner = last tri with zq < z_init            -> max id
//   no Z test       : winner = last covering tri                     -> max id
// Ties on zq resolve to the lower triangle index = the earlier submission,
// exactly as the sequential LESS test would.  So fragments are reduced in any
// order, with 64-bit LDS atomics, and only the winner is shaded (deferred).
//
//   1 k_free_count   tile histogram of (tile, triangle) pairs, aggregated in
//                    LDS per workgroup (one global atomic per touched tile)
//   2 k_free_plan    one workgroup: exclusive scans of the tile counts (list
//                    offsets) and of the slice counts (work items)
//   3 k_free_emit    per-tile lists (order inside a list is irrelevant here)
//   4 k_vis          one 256-thread workgroup per (tile, slice of <= SLICE
//                    triangles; an empty tile is one item): each wave takes
//                    64-triangle chunks, lane = triangle -> exact row spans ->
//                    depth + LDS atomic on the tile's 2048 packed keys; then the same
//                    workgroup shades the tile (deferred: winner ->
//                    barycentrics -> colour -> ApplyPixel -> framebuffer,
//                    depth and u8 frame written once).  A tile whose list is
//                    split over several slices (the load-balancing step for
//                    dense tiles, e.g. mesh poles) merges its keys into `vis`
//                    with global atomics and the last slice to finish shades
//                    it and resets those keys.
//   5 k_keys         an unchanged repeat draw only (key cache): each tile's
//                    final keys, stored by one capture frame's k_vis, are loaded
//                    back into LDS and the tile is shaded as in 4 -- no raster.
// This file is the host side of a batch.  The kernels of 1-3 (and the warm
// binning, the visible list's, the visible plan's and the key plan's) are in
// nr_free_bin.hip, those of 4 and 5 in nr_free_vis.hip; nr_free.h declares
// their launch functions and what host and kernels share.
#include "nr_free.h"
#include "nr_key_records.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace nrtri {
namespace {

using VisStage = TriScratch::Schedule::VisStage;
using ReplanStage = TriScratch::Schedule::ReplanStage;
using KeyStage = TriScratch::Schedule::KeyStage;
using RecStage = TriScratch::Schedule::RecStage;

// Events of a batch carried by the kernels' own completion signals
// (hipExtLaunchKernel stop events) instead of separate marker packets: every
// packet between two rasters on the main queue costs a few microseconds.

// Everything a batch needs to be re-run after an overflow (nr_settle).
struct PendingBatch {
    FrameParams fp;   // (fp.src == bp.src: the batch's arrays)
    BinParams bp;
    int set;
    u32 seq;
    TriangleBuffer* tb;   // non-null: record the validated totals as its known sizes
    BinKey key;
    bool ordered;         // rasterised by the ordered raster (binned)
};

static BinKey bin_key(const BinParams& bp) {
    BinKey k;
    memset(&k, 0, sizeof k);   // padding too: keys are compared bytewise
    for (int i = 0; i < 6; ++i) k.m[i] = bp.m[i];
    k.W = bp.W; k.H = bp.H; k.period = bp.period; k.mask = bp.mask;
    return k;
}

static void record_known(TriangleBuffer* tb, const BinKey& key, const BatchTotals& t) {
    if (!tb) return;
    tb->known = true;
    tb->knownKey = key;
    tb->knownTotals = t;
}


// Binning output sets in rotation: with k sets the binning of batch b waits
// only for the raster of batch b - k.
constexpr int BIN_SETS = 3;

static hipEvent_t sync_event() {
    hipEvent_t e;
    NR_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    return e;
}

// Has everything before event e (or, the twin, on stream s) completed?  Asked
// without waiting.  "Not ready" is an answer, not a failure: its sticky error
// is cleared.  A real asynchronous error is latched.
enum EventState { EV_DONE, EV_PENDING, EV_ERROR };
static EventState query_state(hipError_t q) {
    if (q == hipSuccess) return EV_DONE;
    if (q == hipErrorNotReady) {
        (void)hipGetLastError();
        return EV_PENDING;
    }
    NR_CHECK(q);
    return EV_ERROR;
}
static EventState event_state(hipEvent_t e) { return query_state(hipEventQuery(e)); }
static EventState stream_state(hipStream_t s) { return query_state(hipStreamQuery(s)); }

// A warm binning beside the raster hands off to the raster through its token
// only.  Should the raster's wait time out (a binning delayed by over a second,
// or serialised dispatch), the raster falls back and finishes while that
// binning may still be queued or running on the binning stream, and nothing
// orders later main-stream work after it.  So before the main stream writes a
// binning set or the warm schedule itself -- a binning on the main stream
// (inline warm, or a cold batch binned in line) or sched_capture's copies into
// the schedule every warm binning reads -- it waits for everything enqueued on
// the binning stream so far.  Steady state (always beside, or
// always inline) never takes this wait.
static void main_after_side_binning(RenderContext* ctx) {
    TriScratch& sc = ctx->tri;
    if (!sc.sideGated) return;
    if (!sc.evSide) sc.evSide = sync_event();
    NR_CHECK(hipEventRecord(sc.evSide, nr_bin_stream_for(ctx->device)));
    NR_CHECK(hipStreamWaitEvent(ctx->stream, sc.evSide, 0));
    sc.sideGated = false;
}

// ---- steps shared by the cold (free_enqueue) and warm (warm_enqueue) batches ----
// Start of a batch in binning set F, binned on stream sb: the set's events on
// first use, and a binning on the main stream ordered after any warm binning
// still on the binning stream.
static void set_begin(RenderContext* ctx, TriScratch::FreeSet& F, hipStream_t sb) {
    if (!F.evBin) { F.evBin = sync_event(); F.evVis = sync_event(); }
    if (sb == ctx->stream) main_after_side_binning(ctx);
}

// Scratch of the split tiles (k_vis only): a slice counter per tile, zeroed
// when allocated (main stream; k_vis leaves them zero), and TH * TW key slots
// per slice.  wait: the main stream, whose running raster may still read the
// slots, drained before a regrow (null: the caller has drained it).
static bool grow_fdone(RenderContext* ctx, int ntiles) {
    TriScratch& sc = ctx->tri;
    bool grew;
    if (!sc.fdone.ensure((size_t)ntiles + 1, &grew)) return false;
    if (grew) NR_CHECK(hipMemsetAsync(sc.fdone, 0, sc.fdone.cap * sizeof(u32), ctx->stream));
    return true;
}
static bool grow_kslot(TriScratch& sc, size_t slices, hipStream_t wait) {
    const size_t need = std::max<size_t>(slices, 1) * (TH * TW);
    if (wait && sc.kslot.needs(need)) NR_CHECK(hipStreamSynchronize(wait));
    return sc.kslot.ensure(need);
}

// Hand-off from a binning on the binning stream sb to the raster on the main
// stream sa: the raster waits for F.evBin -- the stop event of the binning's
// last kernel (carried), or a marker recorded here.  (A device-side hand-off
// instead, a polling kernel on the main queue, measured +15 % on an 8-way share
// and needs the two streams on separate hardware queues: removed in round 4;
// warm batches have their own, k_gate_wait.)
static void bin_handoff(TriScratch::FreeSet& F, hipStream_t sb, hipStream_t sa, bool carried) {
    if (sb == sa) return;
    if (!carried) NR_CHECK(hipEventRecord(F.evBin, sb));
    NR_CHECK(hipStreamWaitEvent(sa, F.evBin, 0));
}

// The visibility raster of a batch binned into set F, on the main stream;
// F.evVis (k_vis done reading the set) is the kernel's stop event, or a marker
// when the batch has no work item.
static void vis_tail(RenderContext* ctx, TriScratch::FreeSet& F, const FrameParams& fp, const VisArgs& va, u32 grid) {
    if (grid > 0) {
        FrameParams fpt = fp;   // (timed: the raster stamps itself on the device clock)
        fpt.tstamp = nr_timing_stamp(ctx, NRK_TILE_RASTER);
        launch_vis_any(fpt, ctx->tri, ctx->tri.last, va, grid, ctx->stream, nullptr, F.evVis);
        NR_CHECK(hipGetLastError());
    } else {
        NR_CHECK(hipEventRecord(F.evVis, ctx->stream));
    }
    F.visRecorded = true;
}

// Host view of a plan kernel's totals (k_free_plan*, k_vis_plan): its PW_COUNT words as the
// host read them complete (SeqWords::read).
static BatchTotals plan_totals(const u32* w, u64 n) {   // {n, pairs, items, split, heavy}
    return BatchTotals{n, w[PW_PAIRS], w[PW_ITEMS], w[PW_SPLIT], w[PW_HEAVY]};
}

// Enqueues one batch with binning outputs in set `si`.  exact: read the
// pair/item totals back (host sync) and allocate exactly; otherwise size the
// list from the previous batch, let the plan kernel check it on the device
// and validate later (nr_settle).  pipelined: bin on the device's binning
// stream -- after the raster that last read set `si`, not after everything
// queued before on the main stream -- so that it overlaps the previous
// batch's k_vis (only for immutable inputs: a TriangleBuffer).  ordered: the
// ordered raster's records and list sort, and its raster instead of k_vis.
struct EnqueueMode {
    bool exact = false, pipelined = false, ordered = false;
};
// known: the batch's totals from its buffer's last validated binning under the
// same key (sizes the scratch; null: sized from the last validated batch).
// Returns ENQ_FAIL, ENQ_OK, or (exact, ordered) ENQ_SORTED: a tile list is
// longer than the ordered raster sorts in LDS -- nothing was rasterised; the
// caller takes the global-sort path.
enum { ENQ_FAIL = 0, ENQ_OK = 1, ENQ_SORTED = 2 };
static int free_enqueue(RenderContext* ctx, const FrameParams& fp, const BinParams& bp, int si, const EnqueueMode em,
                        u32* seqOut, const BatchTotals* known = nullptr) {
    const bool exact = em.exact, ordered = em.ordered;
    const TriSrc& src = bp.src;
    hipStream_t sa = ctx->stream;
    hipStream_t sb = em.pipelined ? nr_bin_stream_for(ctx->device) : sa;
    TriScratch& sc = ctx->tri;
    TriScratch::FreeSet& F = sc.fset[si];
    const int ntiles = fp.tiles_x * fp.tiles_y;
    set_begin(ctx, F, sb);
    // the set's buffers are rewritten (binning stream) only after the raster
    // that last read them; a regrow frees them, so the host waits for it then
    if (F.visRecorded && sb != sa) NR_CHECK(hipStreamWaitEvent(sb, F.evVis, 0));
    auto quiesce = [&]() {
        if (F.visRecorded) NR_CHECK(hipEventSynchronize(F.evVis));
    };
    // room for `need` elements of one of the set's arrays
    auto grow = [&](auto& a, size_t need) {
        need = std::max<size_t>(need, 1);
        if (a.needs(need)) quiesce();
        return a.ensure(need);
    };

    // (k_free_plan_r reads and writes the tile arrays as 16-byte vectors up to TILE_ARR)
    const size_t tneed = std::max<size_t>((size_t)ntiles + 1, TILE_ARR);
    if (F.fcnt.needs(tneed)) quiesce();
    bool grew;
    if (!nr_ensure_together({&F.fcnt, &F.foff, &F.fcur}, tneed, &grew)) return ENQ_FAIL;
    if (grew) {   // counters start at zero; k_free_plan re-zeroes them after each use
        NR_CHECK(hipMemsetAsync(F.fcnt, 0, F.fcnt.cap * sizeof(u32), sb));
        NR_CHECK(hipMemsetAsync(F.fcur, 0, F.fcur.cap * sizeof(u32), sb));
    }
    if (!grow_fdone(ctx, ntiles)) return ENQ_FAIL;
    if (!F.dplan) NR_CHECK(hipMalloc(&F.dplan, PW_DEV * sizeof(u32)));
    if (!F.hplan.ensure()) return ENQ_FAIL;
    if (!grow(F.frect, (size_t)src.n)) return ENQ_FAIL;
    // the ordered raster's per-triangle setup records
    if (ordered && !grow(F.frec, (size_t)std::max<i64>(src.n, 1) * ORec)) return ENQ_FAIL;
    const BatchTotals last = sc.last;   // (the last validated batch's, or this batch's known totals)
    size_t cap;
    if (!exact) {
        const u64 est = std::max<u64>(std::max<u64>(std::max<u64>((u64)last.pairs + last.pairs / 4, (u64)src.n * 2), 1u << 20),
                                      known ? known->pairs : 0);
        cap = (size_t)std::min<u64>(sc.capOverride ? sc.capOverride : est, 0xFFFFFFF0ull);
        if (!grow(F.flist, cap)) return ENQ_FAIL;
        if (!sc.capOverride) cap = std::min<size_t>(F.flist.cap, 0xFFFFFFF0ull);
        // work items: at most one per tile + one per full slice of the list,
        // twice that with dense tiles split into row halves (NR_ROW_SPLIT)
        if (!grow(F.fitems, (size_t)ntiles + cap / SLICE_MIN + 2)) return ENQ_FAIL;
        // key slots of split tiles' slices (TH * TW keys each; ordered batches use none): the last validated
        // batch's + 25 %, at least one per tile (a slot per slice is needed only for tiles over the slice
        // length); the plan kernel checks the capacity on the device
        if (!ordered &&
            !grow_kslot(sc, std::max<size_t>(std::max<size_t>((size_t)last.split + last.split / 4, known ? known->split : 0),
                                             std::min<size_t>((size_t)ntiles, 1024)), sa))
            return ENQ_FAIL;
    } else {
        if (!grow(F.flist, 1) || !grow(F.fitems, 1) || (!ordered && !grow_kslot(sc, last.split, sa))) return ENQ_FAIL;
        cap = std::min<size_t>(F.flist.cap, 0xFFFFFFF0ull);
    }

    hipEvent_t e0, e1;
    u32 grid;
    for (int attempt = 0;; ++attempt) {
        nr_timing_begin_on(ctx, NRK_TRI_COUNT, &e0, &e1, sb);
        launch_free_count(bp, F.fcnt, ntiles, F.frect, ordered ? F.frec.p : nullptr, ordered, sb, nullptr);
        NR_CHECK(hipGetLastError());
        nr_timing_end_on(ctx, NRK_TRI_COUNT, e0, e1, sb);

        const u32 seq = ++sc.planSeq;   // (one numbering for the three sets: PendingBatch::seq)
        *seqOut = seq;
        F.hplan.expect(seq);
        nr_timing_begin_on(ctx, NRK_TRI_SCAN, &e0, &e1, sb);
        const u32 icap32 = (u32)std::min<size_t>(F.fitems.cap, 0xFFFFFFF0ull);
        // (an ordered batch uses no key slots, and its lists must fit the raster's LDS sort)
        const u32 kcap32 = ordered ? 0xFFFFFFFFu : (u32)std::min<size_t>(sc.kslot.cap / (TH * TW), 0xFFFFFFF0ull);
        const u32 maxc = ordered ? ORD_SORT_CAP : 0u;
        const u32 sat = sc.splitAt ? sc.splitAt : SPLIT_AT, dsl = sc.dslice ? sc.dslice : DSLICE;
        launch_free_plan(F.fcnt, ntiles, fp.tiles_x, fp.period, fp.mask, F.foff, F.fitems, F.fcur, F.dplan, F.hplan.dev(),
                         (u32)cap, icap32, seq, kcap32, sat, dsl, maxc, ordered, sb, nullptr);
        NR_CHECK(hipGetLastError());
        nr_timing_end_on(ctx, NRK_TRI_SCAN, e0, e1, sb);

        if (!exact) {
            // grid-stride over the items.  The grid need not cover them all,
            // only fill the chip: one workgroup per item of a batch of known
            // totals, else the last validated batch's items + 25 % (>= 1024,
            // the chip's k_vis workgroup slots) -- not the capacity bound, whose
            // surplus workgroups (45 % of a C3 launch, 90 % of an 8-way share's)
            // were dispatched only to exit
            // (two or three items per workgroup in turn: C3 k_vis 138 -> 150 / 157 us,
            // profiles/r03_c3/ab_grid_div.txt)
            u64 g = F.fitems.cap;
            if (known && known->items) g = known->items;
            else if (last.items) g = std::max<u64>((u64)last.items + last.items / 4, 1024);
            grid = (u32)std::min<u64>(std::min<u64>(g, F.fitems.cap), 8192);
            break;
        }
        // exact: read the totals back; if the list or the items did not fit,
        // grow both and bin again (the plan kernel re-zeroed the counters)
        NR_CHECK(hipStreamSynchronize(sb));
        u32 w[PW_COUNT];
        if (!F.hplan.read(w, PW_COUNT)) {
            nr_set_error_msg("triangle batch: plan result missing (stream idle or failed)");
            return ENQ_FAIL;
        }
        const BatchTotals t = sc.last = plan_totals(w, (u64)src.n);
        grid = t.items;
        if (w[PW_FITS]) break;
        if (ordered && w[PW_LONGEST] > ORD_SORT_CAP) return ENQ_SORTED;
        if (attempt > 0 || !grow(F.flist, t.pairs) || !grow(F.fitems, t.items) ||
            (!ordered && !grow_kslot(sc, t.split, sa))) {
            nr_set_error_msg("triangle binning: pair list allocation failed");
            return ENQ_FAIL;
        }
        cap = std::min<size_t>(F.flist.cap, 0xFFFFFFF0ull);
    }

    nr_timing_begin_on(ctx, NRK_TRI_EMIT, &e0, &e1, sb);
    const bool xs = sb != sa && !e1;   // no timing events around the kernel
    hipEvent_t binStop = xs ? F.evBin : nullptr;
    hipEvent_t emitStop = ordered ? nullptr : binStop;   // (ordered: the list sort ends the binning)
    launch_free_emit(bp, F.foff, F.fcur, F.flist, ntiles, F.frect, F.dplan, sb, emitStop);
    NR_CHECK(hipGetLastError());
    nr_timing_end_on(ctx, NRK_TRI_EMIT, e0, e1, sb);
    if (ordered) {   // each tile's list into submission order
        nr_timing_begin_on(ctx, NRK_TRI_SORT, &e0, &e1, sb);
        launch_tile_sort(F.foff, F.flist, F.dplan, ntiles, sb, binStop);
        NR_CHECK(hipGetLastError());
        nr_timing_end_on(ctx, NRK_TRI_SORT, e0, e1, sb);
    }
    bin_handoff(F, sb, sa, xs);

    if (ordered) {   // one workgroup per tile, its list sorted in LDS
        FrameParams fpt = fp;   // (timed: the raster stamps itself on the device clock)
        fpt.tstamp = nr_timing_stamp(ctx, NRK_TILE_RASTER);
        launch_ordered_binned(fpt, F.flist, F.foff, F.dplan, F.frec, ntiles, sa, nullptr, F.evVis);
        NR_CHECK(hipGetLastError());
        F.visRecorded = true;
    } else {
        vis_tail(ctx, F, fp, VisArgs{F.fitems, F.flist, F.dplan, WarmCheck{nullptr, nullptr, nullptr, 0u, 0u, nullptr, 0u}}, grid);
    }
    return ENQ_OK;
}

// ---- warm binning ---------------------------------------------------------
// On unless SetWarmBinning(2).
static bool warm_on(const TriScratch& sc) { return sc.warmMode != 2; }
// Warm binning inline (main stream, right before the raster) or beside the
// previous raster (binning stream).  Inline when the rank's owned share of
// the batch is large and its frame share small: 1M triangles at 1080p
// 0.1001 -> 0.0985 ms per frame; beside the raster for small batches (C2
// 0.065 -> 0.058 ms), for the smaller shares, whose active binning blocks fit
// beside the raster (8-way 0.0505 -> 0.046-0.048 ms, 4-way -1 %;
// profiles/r04/ab_warm_blocks.txt), and -- since the fast clear left the
// raster HBM time to share -- for frame shares of >= 4 M pixels (C3 at 4K
// 0.130 -> 0.124 ms, its 2-way share 0.092 -> 0.077 ms;
// profiles/r05/ab_warm_beside.txt).  NR_WARM_INLINE: 1 always inline, 0
// always beside (A/B); inline by default under AMD_SERIALIZE_KERNEL.
static bool warm_inline(i64 n, int period, u64 mask, i64 W, i64 H) {
    static const int v = [] {
        const char* e = getenv("NR_WARM_INLINE");
        if (e) return atoi(e);
        // serialised dispatch: a binning beside the raster could not start
        // until the raster's token wait gave up (a second per frame)
        const char* ser = getenv("AMD_SERIALIZE_KERNEL");
        return ser && atoi(ser) != 0 ? 1 : 2;
    }();
    if (v != 2) return v != 0;
    const u64 m = period >= 64 ? mask : (mask & ((1ull << period) - 1ull));
    const f64 share = period == 1 ? 1.0 : (f64)__builtin_popcountll(m) / (f64)period;
    if ((f64)W * (f64)H * share >= 4.0e6) return false;
    return n >= 65536 && (f64)n * share >= 300000.0;
}

// Keeps the tile offsets, work items and plan totals of a validated binning
// of `tb` under `key` (binning set F, which held room for them) as the
// context's warm schedule: device copies on the main stream, after the
// batch's raster; the set's next binning waits for them (F.evVis).
static void sched_capture(RenderContext* ctx, TriScratch::FreeSet& F, const BinKey& key, const TriangleBuffer* tb,
                          int ntiles, const BatchTotals& t) {
    TriScratch& sc = ctx->tri;
    if (!warm_on(sc) || !tb) return;
    auto& S = sc.sched;
    hipStream_t sa = ctx->stream;
    main_after_side_binning(ctx);   // (a late warm binning may still read S.off)
    S.valid = false;
    S.listSet = -1;   // (a new generation: no list of its own yet)
    S.drop_visible();
    const size_t ineed = std::max<size_t>(t.items, 1);
    if (S.off.needs((size_t)ntiles + 1) || S.items.needs(ineed) || !S.dplan) {
        NR_CHECK(hipStreamSynchronize(sa));   // a queued warm batch may still read the old arrays
        NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(ctx->device)));
        if (!S.off.ensure((size_t)ntiles + 1) || !S.items.ensure(ineed)) return;
        if (!S.dplan) NR_CHECK(hipMalloc(&S.dplan, PW_DEV * sizeof(u32)));
    }
    if (!S.ready) S.ready = sync_event();
    NR_CHECK(hipMemcpyAsync(S.off, F.foff, ((size_t)ntiles + 1) * sizeof(u32), hipMemcpyDeviceToDevice, sa));
    if (t.items) NR_CHECK(hipMemcpyAsync(S.items, F.fitems, (size_t)t.items * sizeof(uint4), hipMemcpyDeviceToDevice, sa));
    NR_CHECK(hipMemcpyAsync(S.dplan, F.dplan, PW_DEV * sizeof(u32), hipMemcpyDeviceToDevice, sa));
    NR_CHECK(hipEventRecord(S.ready, sa));
    NR_CHECK(hipEventRecord(F.evVis, sa));   // the set is rewritten only after the copies
    F.visRecorded = true;
    S.valid = true;
    S.tbUid = tb->uid;
    S.key = key;
    S.totals = t;
    S.splitAt = sc.splitAt; S.dslice = sc.dslice;   // (the limits the binning was planned under: visible_replan)
    static u64 g_gen = 0;
    S.gen = ++g_gen;
    S.waitReady = true;
}

// A validated binning of `tb` under `key` in set F: its totals are the
// buffer's known sizes, and -- when it fitted, so that the set holds its
// offsets and items -- it becomes the warm schedule.
static void keep_binning(RenderContext* ctx, TriScratch::FreeSet& F, const BinKey& key, TriangleBuffer* tb, int ntiles,
                         const BatchTotals& t, bool fitted = true) {
    record_known(tb, key, t);
    if (fitted) sched_capture(ctx, F, key, tb, ntiles, t);
}

static bool sched_matches(const TriScratch& sc, const TriangleBuffer* tb, const BinKey& key) {
    return warm_on(sc) && tb && sc.sched.valid && sc.sched.tbUid == tb->uid && !sc.capOverride &&
           memcmp(&sc.sched.key, &key, sizeof key) == 0 &&
           std::find(sc.warmBanned.begin(), sc.warmBanned.end(), tb->uid) == sc.warmBanned.end();
}

// Loose binning (round 6): the buffer of the schedule drawn under another
// transform (same frame and shard pattern; any depth mode -- the schedule
// holds binning results only), where no vertex moves more than LOOSE_PX on
// screen from where the schedule's transform put it -- a moving or jittering
// scene.  Every tile's pair count then changes by the
// triangles that cross its edges; the loose ranges (loose_cap) hold them, so
// the batch bins in one pass (k_bin_warm) instead of count -> plan -> emit.
// The displacement bound: the two affine maps differ by an affine map, whose
// largest displacement over the buffer's bounding box is at one of its corners.
constexpr f64 LOOSE_PX = 2.0;
static bool loose_matches(const TriScratch& sc, const TriangleBuffer* tb, const BinKey& key) {
    const auto& S = sc.sched;
    if (!warm_on(sc) || !tb || !S.valid || S.tbUid != tb->uid || sc.capOverride) return false;
    if (S.key.W != key.W || S.key.H != key.H || S.key.period != key.period || S.key.mask != key.mask) return false;
    if (std::find(sc.warmBanned.begin(), sc.warmBanned.end(), tb->uid) != sc.warmBanned.end() ||
        std::find(sc.looseBanned.begin(), sc.looseBanned.end(), tb->uid) != sc.looseBanned.end())
        return false;
    const f64* b = tb->bbox;
    if (!(std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]) && std::isfinite(b[3]))) return false;
    for (int c = 0; c < 4; ++c) {
        const f64 x = b[(c & 1) ? 2 : 0], y = b[(c & 2) ? 3 : 1];
        f64 ax, ay, bx, by;
        nr_xform(S.key.m, x, y, ax, ay);
        nr_xform(key.m, x, y, bx, by);
        if (!(std::fabs(ax - bx) <= LOOSE_PX && std::fabs(ay - by) <= LOOSE_PX)) return false;
    }
    return true;
}

// A warm batch that failed its checks (k_vis WarmCheck: the raster then ran
// over every triangle, so its frame is right) -- read at the next call into
// the context: latch an error, drop the schedule (the next draw bins cold),
// and after a binning-check failure bin that buffer cold from now on.
static void warm_poll(RenderContext* ctx) {
    TriScratch& sc = ctx->tri;
    if (!sc.hfail) return;
    const u32 f = __atomic_load_n(sc.hfail, __ATOMIC_ACQUIRE);
    if (!f) return;
    const u32 w1 = __atomic_load_n(&sc.hfail[1], __ATOMIC_ACQUIRE), w2 = __atomic_load_n(&sc.hfail[2], __ATOMIC_ACQUIRE);
    const u32 w3 = __atomic_load_n(&sc.hfail[3], __ATOMIC_ACQUIRE);
    __atomic_store_n(sc.hfail, 0u, __ATOMIC_RELEASE);
    ++sc.warmFailures;
    char msg[320];
    if (f == 4) {   // a tile over its loose range: the schedule stays, the buffer is not binned loose again
        if (sc.sched.valid) sc.looseBanned.push_back(sc.sched.tbUid);
        snprintf(msg, sizeof msg, "triangle batch: a loose warm binning gave tile %u %u pairs, room for %u; that "
                                  "tile was rasterised from all the batch's triangles and the buffer is no longer "
                                  "binned loose", w1, w2, w3);
        nr_set_error_msg(msg);
        return;
    }
    if (f != 2 && sc.sched.valid) sc.warmBanned.push_back(sc.sched.tbUid);
    sc.sched.valid = false;
    sc.sched.drop_visible();
    if (f == 2)
        snprintf(msg, sizeof msg, "triangle batch: a raster's wait for its warm binning timed out; the batch was "
                                  "rasterised from all its triangles (under serialised kernel dispatch -- a "
                                  "profiler's counter passes, AMD_SERIALIZE_KERNEL -- set NR_WARM_INLINE=1)");
    else if (f == 1)
        snprintf(msg, sizeof msg, "triangle batch: a warm binning put a tile over its range (tag %u of batch %u); the "
                                  "batch was rasterised from all its triangles and the buffer bins cold from now on",
                 w2, w3);
    else
        snprintf(msg, sizeof msg, "triangle batch: a warm binning gave tile %u %u pairs, expected %u; that tile was "
                                  "rasterised from all the batch's triangles and the buffer bins cold from now on",
                 w1, w2, w3);
    nr_set_error_msg(msg);
}

// The binning blocks (256 * TPT triangles) of a schedule with a cluster that
// may reach an owned tile: cluster_may_touch on the host over the buffer's
// cluster boxes with the wider margins CLUSTER_HOST (the device test still
// runs per wave).  Built once per schedule: the warm binning of a rank then
// launches only these workgroups (an 8-way share: about 1 in 7).
static void warm_blocks(RenderContext* ctx, const BinParams& bp, const TriangleBuffer* tb) {
    auto& S = ctx->tri.sched;
    if (S.blocksGen == S.gen) return;
    const i64 n = bp.src.n, per = 256 * TPT, nb = (n + per - 1) / per;
    const i64 nc = (i64)tb->hcbox.size() / 4;
    // (the previous upload from this vector was ordered before any warm
    // binning of the previous schedule, all of which the sync below or the
    // stream order has passed)
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<u32>& act = S.hblocks;
    act.clear();
    act.reserve((size_t)nb);
    bool anyCull = false;
    for (i64 b = 0; b < nb; ++b) {
        bool any = false;
        for (i64 c = b * (per / NR_CLUSTER); c < std::min<i64>((b + 1) * (per / NR_CLUSTER), nc); ++c) {
            const bool t = cluster_may_touch(bp, tb->hcbox.data() + c * 4, CLUSTER_HOST);
            any = any || t;
            anyCull = anyCull || !t;
        }
        if (any || nc == 0) act.push_back((u32)b);
    }
    // every cluster may reach an owned tile (an unsharded frame with the mesh
    // on screen): the device's cluster tests could cull nothing worth a test
    S.anyCull = anyCull;
    if (S.blocks_cap < std::max<size_t>(act.size(), 1)) {
        NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(ctx->device)));
        if (S.blocks) NR_CHECK(hipFree(S.blocks));
        S.blocks_cap = std::max<size_t>((size_t)nb, 1);
        NR_CHECK(hipMalloc(&S.blocks, S.blocks_cap * sizeof(u32)));
    }
    // (ordered on the main stream before any warm binning of this schedule, S.ready)
    if (!act.empty())
        NR_CHECK(hipMemcpyAsync(S.blocks, act.data(), act.size() * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
    NR_CHECK(hipEventRecord(S.ready, ctx->stream));
    S.waitReady = true;
    S.nblocks = (u32)act.size();
    S.blocksGen = S.gen;
}

// ---- visible list -----------------------------------------------------------
// Under list reuse the buffer, the key and the pair list are those of the frame
// before, so the triangles that can win a pixel are too.  One reused batch of a
// schedule generation is the marking frame: its k_vis (a MARK instance) sets
// bit t of S.vmask for every triangle t that wins a pixel.  k_prune_list then
// copies the kept list without the unmarked triangles -- same offsets, each
// tile's order kept -- into S.vlist, with the tiles' kept counts in S.vcnt, and
// later reused batches of that depth mode rasterise from the copy with k_vis
// unchanged: the counts are the cursors of a WarmCheck in the loose format, so
// each item slices its tile's actual count afresh.
// Exact, because the raster is a per-pixel min / max over keys (zq << 32) | id
// and a triangle that wins no pixel changes none ("Visible list"):
//   LESS + write: marked only on a frame whose depth is a pending clear to
//     0xFFFFFFFF; an unmarked triangle's key is above a kept one's at every
//     pixel it covers, whatever the depth buffer holds -- valid for every later
//     LESS + write draw;
//   no test: the highest covering id wins, whatever the depth -- valid for
//     that mode;
//   LESS without write: never pruned (the passing set depends on the depth
//     buffer's contents); such draws, and any draw in a mode other than the
//     capturing one, use the full list, which stays where it is.
// The list is dropped with the schedule generation (sched_capture, a failed
// check, a resize, SetWarmBinning(2), a capacity override).
static bool visible_capture_ok(const FrameParams& fp, int zm) {
    if (fp.fragCounter || fp.src.n <= 0) return false;
    if (zm == 1) return fp.pendDepth && fp.pendDepthValue == 0xFFFFFFFFu;
    return zm == 0;
}

// Items the visible plan can need at most: an item per tile and, over the
// kept pairs (<= the schedule's), a slice per SLICE_MIN of them.
static size_t vitems_need(const BatchTotals& t, int ntiles) {
    return std::max<size_t>((size_t)t.items, (size_t)ntiles + (size_t)t.pairs / SLICE_MIN + 1);
}

// The marking frame's set-up: room for the mask, the pruned list, the counts
// and the visible plan (a regrow waits for the main stream: a queued batch of
// an earlier generation may still read them; first use or a larger schedule),
// the mask zeroed on the main stream, and the batch's snapshot pointed at it.
static void visible_mark_begin(RenderContext* ctx, FrameParams& fp, int ntiles) {
    auto& S = ctx->tri.sched;
    const size_t words = ((size_t)fp.src.n + 31) / 32, pairs = std::max<size_t>(S.totals.pairs, 1);
    const size_t vitems = vitems_need(S.totals, ntiles);
    if (S.vmask.needs(words) || S.vlist.needs(pairs) || S.vcnt.needs((size_t)ntiles + 3) || S.vitems.needs(vitems) ||
        !S.vplan) {
        NR_CHECK(hipStreamSynchronize(ctx->stream));
        if (!S.vmask.ensure(words) || !S.vlist.ensure(pairs) || !S.vcnt.ensure((size_t)ntiles + 3) ||
            !S.vitems.ensure(vitems))
            return;
        if (!S.vplan) NR_CHECK(hipMalloc(&S.vplan, PW_DEV * sizeof(u32)));
        S.hvplan.ensure();   // (no memory: latched, and visible_replan plans nothing)
    }
    NR_CHECK(hipMemsetAsync(S.vmask, 0, words * sizeof(u32), ctx->stream));
    fp.winMask = S.vmask;
}

// After a marking frame: prune once the host has seen, without waiting, that
// the marking frame -- and with it, in stream order, the list's binning frame,
// whose raster checked the binning -- is done, and that no check failed
// (hfail: a failure is latched by the next warm_poll, which drops the
// schedule; a failed list is never pruned).  Main stream, before the batch
// that first reads the pruned list.
static void visible_prune(RenderContext* ctx, int ntiles) {
    TriScratch& sc = ctx->tri;
    auto& S = sc.sched;
    if (S.markSet != S.listSet || S.markTag != S.listTag) {   // binned again since: mark afresh
        S.visState = VisStage::None;
        return;
    }
    const EventState q = event_state(S.evMark);
    if (q == EV_PENDING) return;
    if (q == EV_ERROR) {
        S.visState = VisStage::None;
        return;
    }
    if (sc.hfail && __atomic_load_n(sc.hfail, __ATOMIC_ACQUIRE)) return;
    if (!S.totals.items) return;
    NR_CHECK(hipMemsetAsync(S.vcnt, 0, ((size_t)ntiles + 3) * sizeof(u32), ctx->stream));
    launch_prune_list(S.items, S.totals.items, S.off, sc.fset[S.listSet].flist, S.vmask,
                      (u32)std::min<u64>(S.totals.n, 0xFFFFFFFFull), S.vlist, S.vcnt, S.vcnt.p + ntiles + 2, ctx->stream,
                      nullptr);
    NR_CHECK(hipGetLastError());
    S.visState = VisStage::Pruned;
    S.replanState = ReplanStage::None;
    S.keyState = KeyStage::None;
}

// Visible split limits under test (A/B measurement): NR_VIS_SPLIT_AT /
// NR_VIS_DSLICE replace VIS_SPLIT_AT / VIS_DSLICE; SetSplitLimits still wins.
static u32 vis_limit_env(const char* name, u32 def) {
    const char* e = getenv(name);
    const long v = e ? atol(e) : 0;
    return v > 0 ? (u32)v : def;
}

// The visible plan of the list just pruned (main stream, in stream order after
// k_prune_list and before the first k_vis that reads it).  The schedule's own
// limits, the fall-back on the device, are formed as its plan kernel formed
// them: the slice length from its pair total, the split limits it was binned
// under.
static void visible_replan(RenderContext* ctx, const FrameParams& fp, int ntiles) {
    TriScratch& sc = ctx->tri;
    auto& S = sc.sched;
    if (!S.vplan || !S.hvplan.dev() || S.vitems.cap < vitems_need(S.totals, ntiles)) return;
    static const u32 envAt = vis_limit_env("NR_VIS_SPLIT_AT", VIS_SPLIT_AT);
    static const u32 envDs = vis_limit_env("NR_VIS_DSLICE", VIS_DSLICE);
    const u32 sat = sc.splitAt ? sc.splitAt : envAt, dsl = sc.dslice ? sc.dslice : envDs;
    u32 slice = SLICE_MIN;
    while (slice < SLICE && (u64)slice * SLICE_TARGET < S.totals.pairs) slice <<= 1;
    const u32 lim_s = std::min(slice, S.splitAt ? S.splitAt : SPLIT_AT);
    const u32 dsl_s = std::max<u32>(SLICE_MIN, std::min(lim_s, S.dslice ? S.dslice : DSLICE));
    const u32 lim_p = std::min(slice, sat), dsl_p = std::max<u32>(SLICE_MIN, std::min(lim_p, dsl));
    const u32 icap = (u32)std::min<size_t>(S.vitems.cap, 0xFFFFFFF0ull);
    const u32 kcap = (u32)std::min<size_t>(sc.kslot.cap / (TH * TW), 0xFFFFFFF0ull);
    launch_vis_plan(S.vcnt, S.off, ntiles, fp.tiles_x, fp.period, fp.mask, S.vitems, S.vplan, S.hvplan.dev(), icap, kcap,
                    S.hvplan.next(), lim_p, dsl_p, lim_s, dsl_s, ctx->stream, nullptr);
    NR_CHECK(hipGetLastError());
    S.replanState = ReplanStage::Enqueued;
}

// The visible plan's totals once the host has seen every word of them (no wait).
static bool vplan_seen(TriScratch::Schedule& S) {
    if (S.replanState == ReplanStage::Seen) return true;
    if (S.replanState != ReplanStage::Enqueued) return false;
    u32 v[PW_COUNT];
    if (!S.hvplan.read(v, PW_COUNT)) return false;
    S.vtotals = plan_totals(v, S.totals.n);
    S.replanState = ReplanStage::Seen;
    return true;
}

// ---- key cache: host side -------------------------------------------------------
// The fourth stage of a schedule generation, after "pruned" (and "re-planned"):
//   1 the key items, planned on the device from the kept counts (k_key_plan), in
//     stream order after k_prune_list, on the first batch of the pruned list;
//   2 once the host has seen their totals (no wait), compact slots for the tiles
//     with a kept pair (TH * TW keys each; no memory: the generation stays on the
//     visible list);
//   3 one batch of the pruned list whose draw could also have marked
//     (visible_capture_ok) is the capture frame: an exact frame like any other
//     whose k_vis also stores every shaded tile's final keys;
//   4 once the host has seen that frame complete (an event query, never a wait)
//     and no check failed, such draws are shaded from the cache (k_keys).
// Exact, because the keys are k_vis's own, taken where shade_tile reads them,
// and depend on the buffer (immutable), the binning key (the generation's) and
// the initial depth only: none for the no-test mode (the highest covering id),
// a pending clear to 0xFFFFFFFF for LESS + write -- the one the capture frame had.
// Dropped with the visible list (Schedule::drop_visible).
static bool key_totals_seen(const TriScratch::Schedule& S, u32* tiles, u32* items) {
    u32 w[2];
    if (!S.hkplan.read(w, 2)) return false;
    *tiles = w[0]; *items = w[1];
    return true;
}

// Does a cached Gouraud batch run k_keys_idx?  SetKeyIndex 2: no; 0 (the default): yes, unless NR_KEY_INDEX=2 in
// the environment (A/B runs against k_keys in one build, profiles/key_index/bench_py_ab.txt).
static bool key_index_wanted(int mode) {
    static const bool envOff = [] {
        const char* e = getenv("NR_KEY_INDEX");
        return e && atoi(e) == 2;
    }();
    return mode != 2 && !envOff;
}

// The three arrays of the generation's key index in S.kindex (ktiles slots each).
static KeyIndex key_index_view(const TriScratch::Schedule& S) {
    const size_t tiles = std::max<size_t>(S.ktiles, 1);
    unsigned char* const b = S.kindex.p;
    KeyIndex ki;
    ki.idx = reinterpret_cast<const unsigned short*>(b);
    ki.win = reinterpret_cast<const u32*>(b + tiles * (size_t)(TH * TW) * 2);
    ki.cnt = ki.win + tiles * (size_t)KI_RT;
    return ki;
}

// Does an indexed batch run k_keys_rec?  SetKeyRecords 2: no; 0 (the default): yes, unless NR_KEY_RECORDS=2 in
// the environment (A/B runs against k_keys_idx in one build).  The store is kept either way.
static bool key_records_wanted(int mode) {
    static const bool envOff = [] {
        const char* e = getenv("NR_KEY_RECORDS");
        return e && atoi(e) == 2;
    }();
    return mode != 2 && !envOff;
}

// The record store of a generation whose offsets are enqueued (RecStage::Scanned), for a Gouraud batch of it:
// once the host has seen the total (no wait; it sits in stream order before the capture frame's event, so the
// first cached batch sees it), room for the records -- a regrow waits for the stream: a queued batch of an
// earlier generation may still read them -- and k_key_records, here, behind frame_params.  Batches after this
// one are shaded from the records.  Over the cap, or no memory: the error is cleared, nothing is latched and the
// generation stays on k_keys_idx.
static void key_records_step(RenderContext* ctx, const FrameParams& fp) {
    auto& S = ctx->tri.sched;
    u32 total = 0;
    if (!S.hkrec.read(&total, 1)) return;
    S.recState = RecStage::None;   // (whatever follows, this generation polls no more)
    if (!nrkrec::fits(total, fp.W, fp.H, fp.ipp)) return;
    const size_t need = (size_t)nrkrec::room_doubles(total);
    if (S.krec.needs(need)) {
        NR_CHECK(hipStreamSynchronize(ctx->stream));
        S.krec.release();
        if (hipMalloc((void**)&S.krec.p, need * sizeof(f64)) != hipSuccess) {
            (void)hipGetLastError();
            S.krec.p = nullptr;
            return;
        }
        S.krec.cap = need;
    }
    launch_key_records(fp, S.kkeys, S.ktiles, key_index_view(S).idx, S.roff(), S.krec, ctx->stream);
    NR_CHECK(hipGetLastError());
    S.krecords = total;
    S.recState = RecStage::Ready;
}

static void key_plan(RenderContext* ctx, const FrameParams& fp, int ntiles) {
    auto& S = ctx->tri.sched;
    const size_t tn = std::max<size_t>((size_t)ntiles, 1);
    // (the capture table: the slots' address in the first two words, then a slot per tile -- KeyCaptureTable)
    if (S.kitems.needs(tn) || S.ktile.needs(tn + 2) || !S.kplan || !S.hkplan.dev()) {
        NR_CHECK(hipStreamSynchronize(ctx->stream));   // (a queued batch of an earlier generation may still read them)
        if (!S.kitems.ensure(tn) || !S.ktile.ensure(tn + 2)) { S.keyState = KeyStage::NoMemory; return; }
        if (!S.kplan) NR_CHECK(hipMalloc(&S.kplan, 2 * sizeof(u32)));
        if (!S.hkplan.ensure() || !S.kplan) { S.keyState = KeyStage::NoMemory; return; }
    }
    launch_key_plan(S.vcnt, ntiles, fp.tiles_x, fp.period, fp.mask, S.kitems, S.ktile.p + 2, S.kplan, S.hkplan.dev(),
                    S.hkplan.next(), ctx->stream, nullptr);
    NR_CHECK(hipGetLastError());
    S.keyState = KeyStage::Planned;
}

// One step of the stages above for a batch of the pruned list in depth mode zm;
// fills in va's key-cache fields.  Returns 1 when the batch is the capture frame
// (the caller records S.evKey after it), 2 when it is shaded from the cache.
static int key_cache_step(RenderContext* ctx, const FrameParams& fp, int zm, int ntiles, VisArgs& va) {
    TriScratch& sc = ctx->tri;
    auto& S = sc.sched;
    if (sc.keyMode == 2 || S.keyState == KeyStage::NoMemory) return 0;
    if (S.keyState == KeyStage::None) {
        key_plan(ctx, fp, ntiles);
        return 0;
    }
    if (S.keyState == KeyStage::Planned) {
        if (!key_totals_seen(S, &S.ktiles, &S.knitems)) return 0;
        const size_t need = std::max<size_t>(S.ktiles, 1) * (size_t)(TH * TW);
        if (S.kkeys.needs(need)) {
            NR_CHECK(hipStreamSynchronize(ctx->stream));   // (as key_plan)
            S.kkeys.release();
            if (hipMalloc((void**)&S.kkeys.p, need * sizeof(u64)) != hipSuccess) {
                (void)hipGetLastError();   // no room: not an error, the generation stays on the visible list
                S.kkeys.p = nullptr;
                S.keyState = KeyStage::NoMemory;
                return 0;
            }
            S.kkeys.cap = need;
        }
        // the key index beside the keys.  No room: not an error and nothing latched -- the generation's cached
        // batches run k_keys
        S.kindexed = false;
        S.recState = RecStage::None;
        const size_t ineed = std::max<size_t>(S.ktiles, 1) * KI_SLOT_BYTES;
        if (S.kindex.needs(ineed)) {
            NR_CHECK(hipStreamSynchronize(ctx->stream));   // (as key_plan)
            S.kindex.release();
            if (hipMalloc((void**)&S.kindex.p, ineed) == hipSuccess) {
                S.kindex.cap = ineed;
            } else {
                (void)hipGetLastError();
                S.kindex.p = nullptr;
            }
        }
        // the slots' distinct counts and record offsets (key records), under the same rules
        const size_t rneed = 2 * std::max<size_t>(S.ktiles, 1) + 1;
        if (S.kroff.needs(rneed)) {
            NR_CHECK(hipStreamSynchronize(ctx->stream));   // (as key_plan)
            S.kroff.release();
            if (hipMalloc((void**)&S.kroff.p, rneed * sizeof(u32)) == hipSuccess) {
                S.kroff.cap = rneed;
            } else {
                (void)hipGetLastError();
                S.kroff.p = nullptr;
            }
        }
        // the slots' address into the capture table, in stream order before the capture frame (an 8-byte copy
        // from pageable memory is staged before the call returns)
        NR_CHECK(hipMemcpyAsync(S.ktile.p, &S.kkeys.p, sizeof(u64*), hipMemcpyHostToDevice, ctx->stream));
        S.keyState = KeyStage::Slotted;
    }
    if (S.keyState == KeyStage::Capturing) {
        const EventState q = event_state(S.evKey);
        if (q == EV_PENDING) return 0;
        if (q == EV_ERROR) {
            S.keyState = KeyStage::NoMemory;
            return 0;
        }
        if (sc.hfail && __atomic_load_n(sc.hfail, __ATOMIC_ACQUIRE)) return 0;   // (warm_poll drops the schedule)
        S.keyState = KeyStage::Cached;
    }
    if (!visible_capture_ok(fp, zm)) return 0;
    if (S.keyState == KeyStage::Slotted) {
        va.capture = true;
        return 1;
    }
    va.kkeys = S.kkeys;
    va.kitems = S.kitems;
    va.kplan = S.kplan;
    // a Gouraud batch of a generation that has its index: k_keys_idx, when SetKeyIndex says so
    if (S.kindexed && fp.src.mode == ATTR_GOURAUD && key_index_wanted(sc.keyIndexMode)) {
        va.kindex = key_index_view(S);
        // ... that has its records: k_keys_rec, when SetKeyRecords says so.  A generation whose records are not
        // built yet builds them here, for the batches after this one
        if (S.recState == RecStage::Ready) {
            if (key_records_wanted(sc.keyRecordMode)) {
                va.krec.rec = S.krec;
                va.krec.roff = S.roff();
                va.krec.cached = S.ktiles;   // (the plan's totals, seen at KeyStage::Planned: k_keys_rec's grid
                va.krec.items = S.knitems;   // and its split into cached and empty items)
            }
        } else if (S.recState == RecStage::Scanned) {
            key_records_step(ctx, fp);
        }
    }
    return 2;
}

// ---- deferred stores: host side (nr_common.h DeferredStores) ----------------------
// May this k_keys_idx batch leave its f64 and depth stores pending?  It must write the frame output of every
// owned pixel itself (fp.frameU8: a uniform colour clear is pending and the frame output is on and sized) with
// the empty tiles stamped, and count nothing; then SetDeferredStores decides: 2 (or NR_DEFER_STORES=2 in the
// environment) never, 1 always, 0 by the rule of nr_defer_policy.h.
static bool defer_wanted(const TriScratch& sc, const FrameParams& fp) {
    static const bool envOff = [] {
        const char* e = getenv("NR_DEFER_STORES");
        return e && atoi(e) == 2;
    }();
    if (!fp.frameU8 || !fp.tileStamp || fp.fragCounter || sc.deferMode == 2 || envOff) return false;
    return sc.deferMode == 1 || sc.deferPolicy.allows();
}

// The record of the k_keys_idx batch just enqueued (defer: it ran the KO_FRAME kernel).
static void deferred_record(RenderContext* ctx, const FrameParams& fp, const VisArgs& va, u32 grid, bool wide, int zm,
                            const TriangleBuffer* tb, bool defer) {
    TriScratch& sc = ctx->tri;
    auto& D = sc.deferred;   // (no live record: frame_params resolved it, a batch starts from resolved buffers)
    if (defer) {
        if (!D.snap) D.snap = new DeferredSnapshot();
        DeferredSnapshot& s = *static_cast<DeferredSnapshot*>(D.snap);
        s.fp = fp;
        s.fp.tstamp = nullptr;
        s.va = VisArgs{};
        s.va.kkeys = va.kkeys; s.va.kitems = va.kitems; s.va.kplan = va.kplan; s.va.kindex = va.kindex;
        s.grid = grid;
        s.wide = wide;
        ++sc.deferredBatches;
    }
    D.colour = true;
    D.depth = zm == 1;
    D.stored = !defer;
    D.wasNeeded = false;
    D.tb = tb;
}

// The end of a record with no live half.
static void deferred_end(TriScratch& sc) {
    auto& D = sc.deferred;
    if (!D.wasNeeded) {
        sc.deferPolicy.superseded();
        ++sc.deferSuperseded;
    }
    D.tb = nullptr;
}

// A reused batch of the pruned list in its depth mode zm (reuse_enqueue): the
// visible list, the visible plan and the key cache.  F: the set of the kept
// full list, whose events the batch takes.
static void pruned_enqueue(RenderContext* ctx, const FrameParams& fp, TriScratch::FreeSet& F, int zm, int ntiles,
                           const TriangleBuffer* tb) {
    TriScratch& sc = ctx->tri;
    auto& S = sc.sched;
    const BatchTotals& T = S.totals;
    hipStream_t sa = ctx->stream;
    const WarmCheck wv{S.vcnt + ntiles, S.vcnt, S.off, 1u, 1u, sc.dfail, 1u};
    // The visible plan (above), unless SetVisibleReplan(2): planned
    // once per pruning, here when the list was pruned with the switch
    // off.  Its items and plan words are in stream order before this
    // raster.  The grid is the schedule's until the host has seen the
    // plan's totals (k_vis strides over plan[PW_ITEMS] items, whatever
    // the grid), then the visible item count.
    // NR_VIS_WIDE=1 (A/B): the workgroup-size choice follows the visible
    // dense-tile count; by default it keeps the schedule's (an 8-way C3
    // share measured no gain, profiles/visible_replan/limits_table.md).
    // Only a schedule with split tiles is planned again: the measured
    // gain is the slices and merges no longer scheduled.  Without any,
    // the plan could only reorder the items, and C2 (no split tile, as
    // many items as workgroup slots) measured 2.7 % slower with it than
    // under the schedule's order (profiles/visible_replan/ab_bench.json).
    VisArgs va{S.items, S.vlist, S.dplan, wv};
    u32 grid = std::min<u32>(T.items, 8192);
    if (sc.replanMode != 2 && T.split > 0) {
        if (S.replanState == ReplanStage::None) visible_replan(ctx, fp, ntiles);
        if (S.replanState != ReplanStage::None) {
            va.items = S.vitems;
            va.plan = S.vplan;
            if (vplan_seen(S)) {
                grid = std::min<u32>(std::max<u32>(S.vtotals.items, 1), 8192);
                static const bool visWide = [] {
                    const char* e = getenv("NR_VIS_WIDE");
                    return e && atoi(e) == 1;
                }();
                if (visWide) sc.last.heavy = S.vtotals.heavy;
            }
            ++sc.replannedBatches;
        }
    }
    // The key cache (above), unless SetKeyCache(2): a cached batch is
    // launched like the pruned batch it replaces (vis_tail: the set's
    // event, the raster's timing slot), with a workgroup per key item.
    const int kstep = key_cache_step(ctx, fp, zm, ntiles, va);
    if (kstep == 2) grid = std::min<u32>(std::max<u32>(S.knitems, 1), 8192);
    FrameParams fpk = fp;
    if (kstep == 1) fpk.kcap = reinterpret_cast<const KeyCaptureTable*>(S.ktile.p);
    // Deferred stores: a k_keys_idx batch leaves its record, and when it may (defer_wanted) its f64 and depth
    // stores pending.
    const bool indexed = kstep == 2 && va.kindex.idx;
    const bool wide = indexed && keys_wide(sc.last);
    if (indexed) {
        nr_deferred_resolve(ctx, true, true);   // (nothing to do behind frame_params; before the raster in any case)
        va.defer = defer_wanted(sc, fp);
    }
    vis_tail(ctx, F, fpk, va, grid);
    if (indexed) deferred_record(ctx, fp, va, grid, wide, zm, tb, va.defer);
    if (kstep == 1) {   // the capture frame: its end, for key_cache_step
        if (S.kindex.p && S.kindex.cap >= std::max<size_t>(S.ktiles, 1) * KI_SLOT_BYTES) {
            // the key index from the keys just captured, in stream order: the event below covers both
            const KeyIndex ki = key_index_view(S);
            const bool scan = S.ktiles && S.kroff.p && S.kroff.cap >= 2 * (size_t)S.ktiles + 1 && S.hkrec.ensure();
            launch_key_index(S.kitems, S.kkeys, S.ktiles, const_cast<unsigned short*>(ki.idx), const_cast<u32*>(ki.win),
                             const_cast<u32*>(ki.cnt), scan ? S.kroff.p : nullptr, fp.W, fp.H, fp.tiles_x, sa);
            NR_CHECK(hipGetLastError());
            S.kindexed = true;
            if (scan) {   // the record offsets and their total, behind the index: key_records_step polls for it
                launch_key_record_scan(S.kdist(), S.ktiles, S.roff(), S.hkrec.dev(), S.hkrec.next(), sa);
                NR_CHECK(hipGetLastError());
                S.recState = RecStage::Scanned;
            }
        }
        if (!S.evKey) S.evKey = sync_event();
        NR_CHECK(hipEventRecord(S.evKey, sa));
        S.keyState = KeyStage::Capturing;
    }
    sc.last = T;
    ++sc.reusedBatches;
    ++sc.prunedBatches;
    if (kstep == 2) ++sc.keyCachedBatches;
    if (kstep == 2 && va.kindex.idx) ++sc.keyIndexedBatches;
    if (kstep == 2 && va.krec.rec) ++sc.keyRecordBatches;
}

// List reuse: the schedule's last warm binning left its pair list in set
// S.listSet and nothing has written that set since.  The buffer is
// immutable and the key is the same, so a binning now would write the same
// pairs: rasterise from the kept list -- no binning, no gate, nothing on the
// binning stream, and the set rotation stays where it is.  The raster
// repeats that binning's checks (its tag, cursor multiple and plan words:
// the gate's copy carries a token timeout), so a list whose binning failed
// falls back on every reuse as it did on the binning frame, and reports
// once (warm_report, per tag); once the host has seen the failure the
// schedule is gone (warm_poll).  Stream order puts this raster after the one
// that first waited for the list; vis_tail re-records F.evVis, so the set's
// next binning waits for the last reader.  An injected fault bins.
static void reuse_enqueue(RenderContext* ctx, const FrameParams& fp, int ntiles, const TriangleBuffer* tb) {
    TriScratch& sc = ctx->tri;
    auto& S = sc.sched;
    const BatchTotals& T = S.totals;
    hipStream_t sa = ctx->stream;
    TriScratch::FreeSet& F = sc.fset[S.listSet];
    sc.last = T;
    // The visible list (above): prune after a marking frame the host has
    // seen complete; rasterise from the pruned copy in its depth mode --
    // the schedule's items and plan, the kept counts as the cursors of a
    // loose-format check whose tag (1) never matches its words (always 0);
    // else the full list, on one eligible frame per generation with the
    // winners marked.
    const int zm = z_mode(fp);
    const bool pruning = sc.pruneMode != 2 && !fp.fragCounter;
    if (pruning && S.visState == VisStage::Marking) visible_prune(ctx, ntiles);
    if (pruning && S.visState == VisStage::Pruned && S.visZ == zm) {
        pruned_enqueue(ctx, fp, F, zm, ntiles, tb);
        return;
    }
    FrameParams fpm = fp;
    if (pruning && S.visState == VisStage::None && visible_capture_ok(fp, zm)) visible_mark_begin(ctx, fpm, ntiles);
    const u32* plan = S.listGated ? F.gplan : S.dplan;
    const WarmCheck wc{F.fcur + ntiles, F.fcur, S.off, S.listTag, S.listMult, sc.dfail, 0u};
    vis_tail(ctx, F, fpm, VisArgs{S.items, F.flist, plan, wc}, std::min<u32>(T.items, 8192));
    if (fpm.winMask) {   // a marking frame: its end, for visible_prune
        if (!S.evMark) S.evMark = sync_event();
        NR_CHECK(hipEventRecord(S.evMark, sa));
        S.visState = VisStage::Marking;
        S.visZ = zm;
        S.markSet = S.listSet;
        S.markTag = S.listTag;
    }
    ++sc.reusedBatches;
}

// A warm batch: one binning kernel into the schedule's ranges (binning set
// `si`: cursors and pair list), then k_vis over the schedule's items -- unless
// the schedule's last list can be reused (reuse_enqueue).
// loose: the batch's transform differs from the schedule's (loose_matches):
// bin into the schedule's loose ranges, cursors from 0 (k_bin_warm), and let
// k_vis slice each tile's actual count.
static bool warm_enqueue(RenderContext* ctx, const FrameParams& fp, const BinParams& bp, const TriangleBuffer* tb,
                         bool loose) {
    const f64* tbCbox = tb->cbox;
    TriScratch& sc = ctx->tri;
    auto& S = sc.sched;
    const BatchTotals& T = S.totals;
    hipStream_t sa = ctx->stream;
    hipStream_t sb = warm_inline(bp.src.n, fp.period, fp.mask, fp.W, fp.H) ? sa : nr_bin_stream_for(ctx->device);
    const int ntiles = fp.tiles_x * fp.tiles_y;
    if (!loose && S.listSet >= 0 && sc.reuseMode != 2 && !sc.warmInject) {
        reuse_enqueue(ctx, fp, ntiles, tb);
        return true;
    }
    const int si = sc.fnext;
    sc.fnext = (sc.fnext + 1) % BIN_SETS;
    TriScratch::FreeSet& F = sc.fset[si];
    if (S.listSet == si) S.listSet = -1;   // (rewritten below, or left half grown)
    set_begin(ctx, F, sb);
    if (!sc.hfail) {
        NR_CHECK(hipHostMalloc((void**)&sc.hfail, 4 * sizeof(u32), hipHostMallocMapped | hipHostMallocCoherent));
        for (int k = 0; k < 4; ++k) sc.hfail[k] = 0;
        NR_CHECK(hipHostGetDevicePointer((void**)&sc.dfail, sc.hfail, 0));
    }
    // cursors [0, ntiles), then the batch checks {report tag, error tag} (WarmCheck)
    const size_t tneed = std::max<size_t>((size_t)ntiles + 2, TILE_ARR);
    if (loose && S.off2Gen != S.gen)   // (a bound of the loose list: every tile's loose_cap)
        S.pairs2 = (u64)T.pairs + T.pairs / 4 + 64ull * (u64)(ntiles + 1);
    const size_t lneed = std::max<size_t>(loose ? (size_t)S.pairs2 : (size_t)T.pairs, 1);
    if (loose && lneed >= 0xF0000000ull) return false;
    if (F.fcnt.needs(tneed) || F.flist.needs(lneed) || sc.kslot.needs(std::max<size_t>(T.split, 1) * (TH * TW)) ||
        sc.fdone.needs((size_t)ntiles + 1)) {   // (first use of a set, or a larger schedule: rare)
        NR_CHECK(hipStreamSynchronize(sa));
        NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(ctx->device)));
        bool grew;
        if (!nr_ensure_together({&F.fcnt, &F.foff, &F.fcur}, tneed, &grew)) return false;
        if (grew) {
            NR_CHECK(hipMemsetAsync(F.fcnt, 0, F.fcnt.cap * sizeof(u32), sa));
            F.curGen = 0;
        }
        if (!F.flist.ensure(lneed) || !grow_kslot(sc, T.split, nullptr) || !grow_fdone(ctx, ntiles)) return false;
    }
    // (the active blocks are found under the schedule's own transform: a loose batch launches them all)
    if (tbCbox && !loose) warm_blocks(ctx, bp, tb);
    if (loose && S.off2Gen != S.gen) {   // the schedule's loose ranges, once (main stream, before S.ready)
        if (S.off2.needs((size_t)ntiles + 1)) {
            NR_CHECK(hipStreamSynchronize(sa));
            NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(ctx->device)));
            if (!S.off2.ensure((size_t)ntiles + 1)) return false;
        }
        launch_loose_off(S.off, S.off2, ntiles, sa, nullptr);
        NR_CHECK(hipGetLastError());
        NR_CHECK(hipEventRecord(S.ready, sa));
        S.waitReady = true;
        S.off2Gen = S.gen;
    }
    if (F.visRecorded && sb != sa) NR_CHECK(hipStreamWaitEvent(sb, F.evVis, 0));
    if (S.waitReady && sb != sa) NR_CHECK(hipStreamWaitEvent(sb, S.ready, 0));
    S.waitReady = false;
    // cursors: epoch e of this schedule on this set (k_bin_warm); zeroed for a
    // new schedule, after a cold batch on the set, or before they could wrap
    // (loose: from zero every batch -- they count the tile's pairs)
    if (loose || F.curGen != S.gen || (u64)(F.curEpoch + 1) * std::max<u32>(T.pairs, 1) >= 0xF0000000ull) {
        NR_CHECK(hipMemsetAsync(F.fcur, 0, ((size_t)ntiles + 2) * sizeof(u32), sb));   // (and the check words)
        F.curGen = loose ? 0 : S.gen;
        F.curEpoch = 0;
    }
    const int gb = (int)((bp.src.n + 256 * TPT - 1) / (256 * TPT));
    hipEvent_t e0, e1;
    nr_timing_begin_on(ctx, NRK_TRI_EMIT, &e0, &e1, sb);
    const bool gated = sb != sa && !e1;   // same-queue hand-off (k_gate_wait) instead of an event wait
    if (gated && !F.gate) {
        NR_CHECK(hipMalloc(&F.gate, 4 * sizeof(u32)));
        NR_CHECK(hipMalloc(&F.gplan, PW_DEV * sizeof(u32)));
        // zeroed in order on the signalling stream: a plain hipMemset (null
        // stream) may still be pending when the first signal lands and zero
        // it -- that raster's wait then times out (seen with a cold-batch gate
        // on a busy device, profiles/r05/ab_cold_gate.txt)
        NR_CHECK(hipMemsetAsync(F.gate, 0, 4 * sizeof(u32), sb));
        // and done before the first k_gate_wait (main stream) reads the word:
        // uninitialised memory holding a token would let the raster go early
        // (once per set)
        NR_CHECK(hipStreamSynchronize(sb));
        F.gateTok = 0;
    }
    const bool xs = sb != sa && !e1 && !gated;
    hipEvent_t binStop = xs ? F.evBin : nullptr;
    const u32 epoch = loose ? 0u : F.curEpoch++;
    if (++sc.warmTag == 0) sc.warmTag = 1;
    const u32 tag = sc.warmTag;
    u32* const wstat = F.fcur + ntiles;   // {report tag, error tag} (WS_REP, WS_TAG)
    const int inject = sc.warmInject;
    sc.warmInject = 0;
    // cluster culling of the rank's tile rows, and only the schedule's active blocks launched
    const f64* cbox = S.anyCull || loose ? tbCbox : nullptr;
    const bool useBlocks = cbox && !loose && S.blocksGen == S.gen;
    const u32* const binOff = loose ? S.off2 : S.off;
    const u32* blocks = useBlocks ? S.blocks : nullptr;
    const int grid = useBlocks ? (int)S.nblocks : gb;
    if (inject == 4 && gated) launch_delay_binning(sb, nullptr);
    if (grid > 0) {
        launch_bin_warm(bp, binOff, F.fcur, F.flist, wstat, tag, epoch, cbox, blocks, (u32)inject, (u32)loose, grid, sb,
                        binStop);
    } else if (binStop) {
        NR_CHECK(hipEventRecord(F.evBin, sb));
    }
    NR_CHECK(hipGetLastError());
    nr_timing_end_on(ctx, NRK_TRI_EMIT, e0, e1, sb);
    const u32* visPlan = S.dplan;
    if (gated) {
        if (++F.gateTok == 0) F.gateTok = 1;   // (the word starts at 0)
        if (inject != 2)   // (2: the token is withheld -- tests of the timeout)
            launch_gate_signal(F.gate, F.gateTok, sb, nullptr);
        launch_gate_wait(F.gate, F.gateTok, S.dplan, F.gplan, sa, nullptr);
        NR_CHECK(hipGetLastError());
        visPlan = F.gplan;
        sc.sideGated = true;
    } else {
        bin_handoff(F, sb, sa, xs);
    }
    sc.last = T;   // this batch's totals pick the k_vis variant (launch_vis)
    const WarmCheck wc{wstat, F.fcur, binOff, tag, epoch + 1, sc.dfail, (u32)loose};
    vis_tail(ctx, F, fp, VisArgs{S.items, F.flist, visPlan, wc}, std::min<u32>(T.items, 8192));
    if (!loose) {   // the list later batches under this key reuse
        S.listSet = si;
        S.listTag = tag;
        S.listMult = epoch + 1;
        S.listGated = gated;
    }
    return true;
}

}  // namespace

// ordered: the batch is rasterised by the ordered raster (blending, Z test
// without write...): the same binning, each tile's list sorted in LDS.
void draw_free(RenderContext* ctx, const Batch& b, bool ordered) {
    TriangleBuffer* const tb = b.tb;
    FrameParams fp = frame_params(ctx, b);
    if (ctx->frameOutput && fp.pendColor) {
        const size_t n = (size_t)nr_frame_bytes(ctx);
        if (n <= ctx->frameU8cap) fp.frameU8 = ctx->frameU8;
    }
    if (!ordered && (fp.pendColor || fp.pendDepth))   // fast clear: the empty tiles' clears stay pending (k_vis)
        fp.tileStamp = tile_stamps(ctx, (i64)fp.tiles_x * fp.tiles_y), fp.tileEpoch = ctx->tileEpoch;
    const BinParams bp = bin_params(fp);
    // fragment counting reads a counter back anyway: run exact (synchronous);
    // so does a batch from the caller's device arrays: a deferred overflow
    // re-run (settle, at the next call) could read them after the caller has
    // synchronised and released or rewritten them
    const bool exact = fp.fragCounter != nullptr || b.callerOwned;
    TriScratch& sc = ctx->tri;
    // A TriangleBuffer drawn again under the binning key of its last validated
    // draw has the same pair total: the list is sized to hold it, so the plan's
    // capacity check cannot fail and the batch needs no validation (no host
    // wait for its plan kernel at the next call: the host runs ahead).
    const BinKey key = bin_key(bp);
    // Only unsharded batches: a sharded frame's raster is short, and a binning
    // chain issued at once runs beside it and is starved (measured: 1 GPU C3
    // 0.1640 -> 0.1614 ms, C2 0.0685 -> 0.062 ms with known sizes; an emulated
    // rank share of 4 / 8 shards 0.066 -> 0.076 / 0.054 -> 0.062 ms, where the
    // host wait on the plan paces the binning; profiles/r02_c3/ab_known.txt).
    // (ordered batches are always validated: their plan also checks the list lengths)
    const bool known = !ordered && fp.period == 1 && tb && tb->known &&
                       !sc.capOverride && memcmp(&tb->knownKey, &key, sizeof key) == 0;
    if (known && !exact) {   // this batch's totals pick the k_vis variant (launch_vis)
        sc.last = tb->knownTotals;
        sc.last.n = (u64)fp.src.n;
    }
    // warm: the schedule kept from this buffer's last validated binning under
    // this key, or (loose) under a key whose transform is within LOOSE_PX
    warm_poll(ctx);
    if (!ordered && !exact) {
        const bool same = sched_matches(sc, tb, key);
        const bool loose = !same && loose_matches(sc, tb, key);
        if ((same || loose) && warm_enqueue(ctx, fp, bp, tb, loose)) {
            ctx->lastPath = 1;
            ++sc.warmBatches;
            if (loose) ++sc.looseBatches;
            finish_batch(ctx, fp);
            return;
        }
        if (same) return;   // (error latched; a loose batch that could not be enqueued bins cold)
    }
    const int si = sc.fnext;
    sc.fnext = (sc.fnext + 1) % BIN_SETS;
    u32 seq = 0;
    static const bool pipeOn = [] {   // NR_BIN_PIPE=0: bin on the main stream (A/B, isolated kernel times)
        const char* e = getenv("NR_BIN_PIPE");
        return e ? atoi(e) != 0 : true;
    }();
    // A batch issued to an idle main stream (the first frame after a readback
    // or a Flush) has no raster to overlap its binning with: it bins in line
    // on the main stream, with the wide plan kernel, and k_vis follows without
    // a cross-queue wait (whose wake-up took ~15 us in the kernel trace,
    // profiles/r02h_c3).
    bool idle = false;
    if (pipeOn && tb != nullptr && !exact) idle = stream_state(ctx->stream) == EV_DONE;
    TriScratch::FreeSet& F = sc.fset[si];
    F.curGen = 0;   // (its cursors will hold this batch's counts)
    if (sc.sched.listSet == si) sc.sched.listSet = -1;   // (and its list this batch's pairs)
    EnqueueMode em;
    em.exact = exact;
    em.pipelined = pipeOn && tb != nullptr && !exact && !idle;
    em.ordered = ordered;
    const int r = free_enqueue(ctx, fp, bp, si, em, &seq, known ? &tb->knownTotals : nullptr);
    if (r == ENQ_FAIL) return;
    if (r == ENQ_SORTED) {   // (exact) a tile list too long for the LDS sort
        fp.tileStamp = nullptr;   // (the ordered raster writes every tile)
        draw_ordered_sorted(ctx, fp, bp);
        return;
    }
    const int ntiles = fp.tiles_x * fp.tiles_y;
    if (exact) {
        if (!ordered) keep_binning(ctx, F, key, tb, ntiles, sc.last);
    } else if (known) {
        sched_capture(ctx, F, key, tb, ntiles, sc.last);
    } else {
        PendingBatch* pb = new PendingBatch{fp, bp, si, seq, tb, key, ordered};
        ctx->pendingBatch = pb;
    }
    ctx->lastPath = ordered ? 2 : 1;
    finish_batch(ctx, fp);
}

// Validates the last asynchronously sized batch of `ctx`: waits for its plan
// kernel (usually long finished), and if the pair list did not fit, re-runs
// the batch with an exact allocation.  Called at the start of every API
// entry point that enqueues work on, or reads, the context's buffers, so the
// re-run is ordered before anything that depends on the batch.
void settle(RenderContext* ctx) {
    warm_poll(ctx);
    PendingBatch* pb = reinterpret_cast<PendingBatch*>(ctx->pendingBatch);
    if (!pb) return;
    ctx->pendingBatch = nullptr;
    TriScratch& sc = ctx->tri;
    TriScratch::FreeSet& F = sc.fset[pb->set];
    // wait for the batch's plan (usually long finished): it writes its totals
    // into pinned host memory, each word tagged with the batch's sequence
    // number -- polling them avoids an event record per batch (each costs a
    // multi-microsecond bubble on the stream)
    F.hplan.expect(pb->seq);   // (as free_enqueue left it: no plan has gone into the set since)
    u32 w[PW_COUNT];
    for (u64 spin = 0; !F.hplan.read(w, PW_COUNT); ++spin) {
        if ((spin & 1023) == 1023) {
            const bool idle = hipStreamQuery(ctx->stream) != hipErrorNotReady &&
                              hipStreamQuery(nr_bin_stream_for(ctx->device)) != hipErrorNotReady;
            if (idle && !F.hplan.read(w, PW_COUNT)) {
                nr_set_error_msg("triangle batch: plan result missing (stream idle or failed)");
                delete pb;
                return;
            }
            std::this_thread::yield();
        }
    }
    const int ntiles = pb->fp.tiles_x * pb->fp.tiles_y;
    const bool fits = w[PW_FITS] != 0;
    sc.last = plan_totals(w, (u64)pb->fp.src.n);
    // exact totals, fitted or not; fitted: its offsets and items are the buffer's schedule under this key
    if (!pb->ordered) keep_binning(ctx, F, pb->key, pb->tb, ntiles, sc.last, fits);
    if (!fits) {
        // overflow (or, ordered, a tile list too long for the LDS sort): the
        // batch's later kernels did nothing; re-run it exactly on the main
        // stream, after everything queued so far
        NR_CHECK(hipEventSynchronize(F.evVis));
        u32 seq = 0;
        const bool sorted = pb->ordered && w[PW_LONGEST] > ORD_SORT_CAP;
        EnqueueMode em;
        em.exact = true;
        em.ordered = pb->ordered;
        int rr = ENQ_SORTED;
        if (sorted || (rr = free_enqueue(ctx, pb->fp, pb->bp, pb->set, em, &seq)) == ENQ_SORTED)
            rerun_ordered_sorted(ctx, pb->fp, pb->bp);   // (the context's flags are left as they are now)
        else if (rr == ENQ_OK && !pb->ordered)   // the exact re-run's binning is the buffer's schedule under this key
            keep_binning(ctx, F, pb->key, pb->tb, ntiles, sc.last);
    }
    delete pb;
}

// Pairs kept in the context's visible list, 0 when it has none (waits for the
// main stream: a query, not a draw).
i64 visible_pairs(RenderContext* ctx) {
    auto& S = ctx->tri.sched;
    if (!S.valid || S.visState != VisStage::Pruned) return 0;
    const i64 ntiles = ((S.key.W + TW - 1) / TW) * ((S.key.H + TH - 1) / TH);
    u32 v = 0;
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    NR_CHECK(hipMemcpy(&v, S.vcnt.p + ntiles + 2, sizeof v, hipMemcpyDeviceToHost));
    return (i64)v;
}

// Totals of the context's visible plan -- pairs, work items, slices of split
// tiles, dense tiles -- false when it has none (waits for the main stream).
bool visible_plan_totals(RenderContext* ctx, i64* out) {
    auto& S = ctx->tri.sched;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!S.valid || S.visState != VisStage::Pruned || S.replanState == ReplanStage::None) return false;
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    if (!vplan_seen(S)) return false;
    out[0] = S.vtotals.pairs; out[1] = S.vtotals.items; out[2] = S.vtotals.split; out[3] = S.vtotals.heavy;
    return true;
}

// Totals of the context's key cache -- cached tiles, key items, bytes of the
// cached keys -- false when its items have not been planned (waits for the main
// stream).
bool key_cache_totals(RenderContext* ctx, i64* out) {
    auto& S = ctx->tri.sched;
    out[0] = out[1] = out[2] = 0;
    if (!S.valid || S.visState != VisStage::Pruned || S.keyState == KeyStage::NoMemory || S.keyState == KeyStage::None)
        return false;
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    u32 tiles = 0, items = 0;
    if (!key_totals_seen(S, &tiles, &items)) return false;
    out[0] = tiles; out[1] = items; out[2] = (i64)tiles * (TH * TW) * (i64)sizeof(u64);
    return true;
}

// Totals of the generation's key index -- indexed tiles, staged winners (the
// sum of the slots' counts), KI_DIRECT pixels, bytes of the index -- false while
// the generation has none (waits for the main stream).
bool key_index_totals(RenderContext* ctx, i64* out) {
    auto& S = ctx->tri.sched;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!S.valid || S.visState != VisStage::Pruned || !S.kindexed ||
        (S.keyState != KeyStage::Capturing && S.keyState != KeyStage::Cached))
        return false;
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<u32> cnt(2 * (size_t)S.ktiles);
    if (S.ktiles)
        NR_CHECK(hipMemcpy(cnt.data(), key_index_view(S).cnt, cnt.size() * sizeof(u32), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < S.ktiles; ++s) { out[1] += cnt[2 * s]; out[2] += cnt[2 * s + 1]; }
    out[0] = S.ktiles;
    out[3] = (i64)S.ktiles * (i64)KI_SLOT_BYTES;
    return true;
}

// Totals of the generation's key records -- slots, records, bytes of records -- false while the generation has
// none (waits for the main stream).
bool key_record_totals(RenderContext* ctx, i64* out) {
    auto& S = ctx->tri.sched;
    out[0] = out[1] = out[2] = 0;
    if (!S.valid || S.visState != VisStage::Pruned || !S.kindexed || S.keyState != KeyStage::Cached ||
        S.recState != RecStage::Ready)
        return false;
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    out[0] = S.ktiles;
    out[1] = (i64)S.krecords;
    out[2] = (i64)nrkrec::bytes(S.krecords);
    return true;
}

// Something needs the context's framebuffer (color) and / or depth buffer (depth): the record's live halves among
// them are written now, if the batch had left them pending, and are dead either way.
void deferred_resolve(RenderContext* ctx, bool color, bool depth) {
    TriScratch& sc = ctx->tri;
    auto& D = sc.deferred;
    const bool c = color && D.colour, d = depth && D.depth;
    if (!c && !d) return;
    if (!D.stored && D.snap) {
        const DeferredSnapshot& s = *static_cast<const DeferredSnapshot*>(D.snap);
        hipEvent_t a, b;
        nr_timing_begin(ctx, NRK_FILL, &a, &b);
        launch_keys_resolve(s.fp, s.va, s.grid, s.wide, c, d, ctx->stream);
        NR_CHECK(hipGetLastError());
        nr_timing_end(ctx, NRK_FILL, a, b);
        ++sc.deferResolves;
    }
    if (!D.wasNeeded) {
        D.wasNeeded = true;
        sc.deferPolicy.needed(!D.stored);
    }
    if (c) D.colour = false;
    if (d) D.depth = false;
    if (!D.live()) deferred_end(sc);
}

// A clear has overwritten every value of the framebuffer (color) or of the depth buffer (depth).
void deferred_supersede(RenderContext* ctx, bool color, bool depth) {
    auto& D = ctx->tri.deferred;
    if (!D.live()) return;
    if (color) D.colour = false;
    if (depth) D.depth = false;
    if (!D.live()) deferred_end(ctx->tri);
}

}  // namespace nrtri

void nr_deferred_resolve(RenderContext* ctx, bool color, bool depth) { nrtri::deferred_resolve(ctx, color, depth); }
void nr_deferred_supersede(RenderContext* ctx, bool color, bool depth) { nrtri::deferred_supersede(ctx, color, depth); }
void nr_deferred_drop(RenderContext* ctx) {   // (the contents are discarded: the rule hears nothing)
    auto& D = ctx->tri.deferred;
    D.colour = D.depth = false;
    D.tb = nullptr;
}
void nr_deferred_free(RenderContext* ctx) {
    nr_deferred_drop(ctx);
    delete static_cast<nrtri::DeferredSnapshot*>(ctx->tri.deferred.snap);
    ctx->tri.deferred.snap = nullptr;
}

