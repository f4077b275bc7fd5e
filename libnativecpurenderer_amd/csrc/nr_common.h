// nr_common.h — shared types and device helpers of the MI355X raster library.
//
// Every device helper restates one reference routine bit for bit
// (/root/reference/src/libNativeCPURenderer.cpp:<lines> cited per helper).
// The whole library is compiled with -ffp-contract=off: the reference build
// has no FMA, so neither may we.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include <climits>
#include "nr_defer_policy.h"

typedef long i64;
typedef double f64;
typedef unsigned char iu8;
typedef uint32_t u32;

// ---------------------------------------------------------------------------
// error latch (no exceptions cross the ABI; SURVEY §8b "Errors")
// ---------------------------------------------------------------------------
void nr_set_error(const char* where, hipError_t e);
void nr_set_error_msg(const char* msg);
#define NR_CHECK(call)                                              \
    do {                                                            \
        hipError_t nr_e_ = (call);                                  \
        if (nr_e_ != hipSuccess) nr_set_error(#call, nr_e_);        \
    } while (0)

// ---------------------------------------------------------------------------
// host objects
// ---------------------------------------------------------------------------
struct NRState { f64 m[6]; f64 ct[4]; };
typedef unsigned long long u64;

// Binning geometry of a draw: the positions' transform, the frame and the
// owned tile rows.  The same buffer binned under the same key gives the same
// (tile, triangle) pairs, work items and dense tiles.
struct BinKey {
    f64 m[6];
    i64 W, H;
    int period;
    u64 mask;
};

// A device array grown on demand (never shrunk): pointer and capacity in
// elements.  Converts to the pointer (a template that deduces its argument
// types -- hipExtLaunchKernelGGL, hipcub -- takes `.p`).  No destructor: the
// owner's release() calls release(), with the device set.
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t cap = 0;
    operator T*() const { return p; }
    // would ensure(n) reallocate (and so free memory the device may still read)?
    bool needs(size_t n) const { return !p || cap < n; }
    inline bool ensure(size_t n, bool* grew = nullptr);
    void release() {
        if (p) NR_CHECK(hipFree(p));
        p = nullptr; cap = 0;
    }
};
// Room for n elements in each of K arrays of one capacity (only ever grown
// here, together): a regrow frees them all and allocates max(n, 3/2 capacity)
// each, contents lost (*grew).  False: hipMalloc failed (latched, capacity 0).
template <class T, size_t K>
bool nr_ensure_together(DevArray<T>* const (&a)[K], size_t n, bool* grew = nullptr) {
    if (grew) *grew = false;
    if (!a[0]->needs(n)) return true;
    const size_t cap = a[0]->cap, m = n > cap * 3 / 2 ? n : cap * 3 / 2;
    for (DevArray<T>* x : a) x->release();
    for (DevArray<T>* x : a)
        if (hipMalloc((void**)&x->p, m * sizeof(T)) != hipSuccess) {
            nr_set_error_msg("triangle scratch: hipMalloc failed");
            for (DevArray<T>* y : a) y->cap = 0;
            return false;
        }
    for (DevArray<T>* x : a) x->cap = m;
    if (grew) *grew = true;
    return true;
}
template <class T>
inline bool DevArray<T>::ensure(size_t n, bool* grew) {
    DevArray<T>* const one[1] = {this};
    return nr_ensure_together(one, n, grew);
}

// Tagged host words: 8 pinned, coherent, device-mapped u64 words (one 64-byte
// line) in which a plan kernel leaves its totals for the host, word k =
// (seq << 32) | value.  The device stores each word on its own (8-byte stores
// are single-copy atomic), so a set of totals is complete once every word
// carries the sequence number the host expects.  The words start at 0, so 0 is
// never a sequence number.
struct SeqWords {
    u64* h = nullptr;   // host address (null: not allocated)
    u64* d = nullptr;   // its device address
    u32 seq = 0;        // the number the host expects: its own (next), or one handed in (expect)
    // allocated and zeroed on first use; false: no memory (the error is latched)
    bool ensure() {
        if (!h) {
            NR_CHECK(hipHostMalloc((void**)&h, 8 * sizeof(u64), hipHostMallocMapped | hipHostMallocCoherent));
            if (!h) return false;
            for (int k = 0; k < 8; ++k) h[k] = 0;
        }
        if (!d) NR_CHECK(hipHostGetDevicePointer((void**)&d, h, 0));
        return d != nullptr;
    }
    u64* dev() const { return d; }
    u32 next() {
        if (++seq == 0) seq = 1;
        return seq;
    }
    void expect(u32 s) { seq = s; }   // (a numbering kept outside: TriScratch::planSeq, shared by the binning sets)
    // the low halves of the first n words; true only if every one carries seq (out is whole only then)
    bool read(u32* out, int n) const {
        if (!h) return false;
        for (int k = 0; k < n; ++k) {
            const u64 x = __atomic_load_n(&h[k], __ATOMIC_ACQUIRE);
            if ((u32)(x >> 32) != seq) return false;
            out[k] = (u32)x;
        }
        return true;
    }
    void release() {
        if (h) NR_CHECK(hipHostFree(h));
        h = d = nullptr;
    }
};

// Totals of one binned triangle batch (the plan kernel's, nr_free_bin.hip).
struct BatchTotals {
    u64 n = 0;       // triangles (0: no batch yet)
    u32 pairs = 0;   // (tile, triangle) pairs
    u32 items = 0;   // k_vis work items
    u32 split = 0;   // slices of split tiles (key slots)
    u32 heavy = 0;   // dense tiles (k_vis workgroup size)
};

// Scratch of the triangle pipeline, grown on demand (never shrunk).  Each
// struct's release() frees all it declares (DestroyRenderContext, streams idle).
struct TriangleBuffer;
struct TriScratch {
    DevArray<u64> cnt, off;                                             // per triangle (grown together)
    DevArray<f64> orec;   // ordered raster: per-triangle setup records (ORec doubles each)
    DevArray<u32> keys[2], vals[2];                                     // pairs (grown together)
    DevArray<u32> tile_start, tile_end;                                 // per tile (grown together)
    void* temp = nullptr; size_t temp_bytes = 0;                        // hipcub scratch
    u64* h_total = nullptr;                 // pinned readback: [0] pairs, [1] last count, [2] fragments, [3] opacity
    u64* totals() {                         // h_total, allocated on first use (null: hipHostMalloc failed, latched)
        if (!h_total) NR_CHECK(hipHostMalloc((void**)&h_total, 4 * sizeof(u64)));
        return h_total;
    }
    u64* d_frag = nullptr;                  // device fragment counter
    u32* d_flag = nullptr;                  // device non-opaque flag
    // visibility-buffer raster (nr_tri_free.hip).  The binning outputs are
    // double-buffered (FreeSet): a batch drawn from a TriangleBuffer is binned
    // on the device's binning stream while the previous batch's k_vis runs.
    struct FreeSet {
        DevArray<u32> fcnt, foff, fcur;     // per tile (grown together)
        DevArray<uint4> fitems;
        DevArray<u64> frect;                // per-triangle tile rectangle (count -> emit)
        DevArray<f64> frec;                 // ordered batches: per-triangle setup records (ORec doubles each)
        DevArray<u32> flist;
        u32* dplan = nullptr;
        SeqWords hplan;                     // host copy of the plan totals (PW_COUNT words), numbered by planSeq
        hipEvent_t evBin = nullptr;         // binning done (binning stream)
        hipEvent_t evVis = nullptr;         // k_vis done reading the set (main stream)
        bool visRecorded = false;
        u64 curGen = 0;                     // fcur = curEpoch x the counts of schedule curGen (0: unknown)
        u32 curEpoch = 0;
        // warm binning beside the raster: same-queue hand-off (k_gate_signal / k_gate_wait)
        u32* gate = nullptr;                // [0] token of the set's last finished binning
        u32* gplan = nullptr;               // the raster's plan words (k_gate_wait copies the schedule's)
        u32 gateTok = 0;
        void release() {
            fcnt.release(); foff.release(); fcur.release(); fitems.release(); frect.release(); frec.release(); flist.release();
            if (dplan) NR_CHECK(hipFree(dplan));
            if (gate) NR_CHECK(hipFree(gate));
            if (gplan) NR_CHECK(hipFree(gplan));
            hplan.release();
            if (evBin) NR_CHECK(hipEventDestroy(evBin));
            if (evVis) NR_CHECK(hipEventDestroy(evVis));
        }
    } fset[3];
    int fnext = 0;                          // set of the next batch
    DevArray<u32> fdone;                    // split-tile slice counters (k_vis only)
    DevArray<u64> kslot;                    // split-tile key slots, TH*TW keys per slice (k_vis)
    u32 planSeq = 0;                        // sequence number of the last async plan
    BatchTotals last;                       // the last validated batch's: the next one's estimates, the k_vis variant
    u64 capOverride = 0;                    // testing: force this pair capacity
    int coopMode = 0;                       // k_vis variant: 0 auto, 1 coop, 2 lane-only (SetCoopRaster)
    u32 splitAt = 0, dslice = 0;            // dense-tile split limits (SetSplitLimits; 0: NR_SPLIT_AT / NR_DSLICE)
    DevArray<f64> stage;                    // DrawTriangles() with host arrays
    // DrawMesh (nr_mesh.hip): the draw's transformed vertices and assembled soup -- (x, y) nv*2, z nv (padded
    // to an even count), xy n*6, z n*3; read by the batch until it is settled, like `stage`.  A perspective
    // textured draw (SetMeshPerspective) adds the vertices' 1/w, nv padded like z, before the soup and the
    // soup's q n*3 after its z.  A lit draw (DrawMeshLit, DESIGN.md §3 "Vertex lighting") also keeps its
    // per-vertex lit colours here (nv*4, K*nv*4 instanced) and the soup's attributes gathered from them
    DevArray<f64> mstage;
    // clipped / culled mesh draws (nr_mesh.hip, SetMeshNearPlane / SetMeshCull): the draw's clip coordinates
    // (cx, cy, cz, cw) nv*4, and per source triangle its keep mask | output count | scanned offset, n each
    // (+ the total); the emitted soup -- xy n_out*6, z n_out*3 (padded to an even count), attributes
    // n_out*attr_stride, and a perspective textured draw's q n_out*3 -- is then what mstage holds
    DevArray<f64> mclip;
    DevArray<u32> mscan;
    // instanced mesh draws (nr_mesh.hip, DrawMeshInstanced): the draw's K matrices (K*16) and, behind them, its
    // tints (K*4) and a lit draw's normal matrices (K*9) on the device, overwritten only after settle like mstage; a host call's arrays reach it through
    // one of the two pinned h_minst, in turn, by an asynchronous copy (evMinst: that copy is done, the buffer
    // may be rewritten)
    DevArray<f64> minst;
    f64* h_minst[2] = {nullptr, nullptr}; size_t h_minst_cap[2] = {0, 0};
    hipEvent_t evMinst[2] = {nullptr, nullptr};
    int minstNext = 0;
    // warm binning (nr_tri_free.hip): the tile offsets, k_vis work items and
    // plan totals of the last validated binning of one TriangleBuffer under
    // one binning key -- a later draw of the same buffer under the same key
    // has the same (tile, triangle) pairs, so it bins in one pass into these
    // ranges (no count pass, no plan, no validation)
    struct Schedule {
        bool valid = false;
        u64 tbUid = 0;
        BinKey key;
        DevArray<u32> off;                               // ntiles + 1 list offsets
        DevArray<uint4> items;                           // k_vis work items
        u32* dplan = nullptr;                            // the plan's device totals {pairs, items, slices, fits}
        BatchTotals totals;
        u64 gen = 0;                                     // process-unique generation of this schedule
        hipEvent_t ready = nullptr;                      // the copies above are done (main stream)
        bool waitReady = false;                          // the next warm binning on the binning stream waits for it
        // the binning blocks (1024 triangles) with a cluster that may reach an
        // owned tile under this key: the warm binning launches only those
        u32* blocks = nullptr; size_t blocks_cap = 0;
        std::vector<u32> hblocks;                        // (host source of the last upload, kept alive)
        u32 nblocks = 0;
        u64 blocksGen = 0;                               // gen the list was built for (0: none)
        bool anyCull = true;                             // some cluster may lie off the owned tiles (else no device test)
        // loose ranges (round 6): every tile's range widened to loose_cap(count)
        // pairs, for a draw of the same buffer under a transform that moves no
        // vertex more than LOOSE_PX from the key's (a moving scene: k_bin_warm
        // into these ranges, k_vis slices each tile's actual count)
        DevArray<u32> off2;                              // ntiles + 1 loose list offsets
        u64 off2Gen = 0;                                 // gen they were formed for (0: none)
        u64 pairs2 = 0;                                  // a bound of off2[ntiles] (list capacity)
        // list reuse: the binning set that holds the pair list (and cursors) of this
        // generation's last warm binning, untouched since (-1: none), and that
        // batch's checks -- a later batch under the same key rasterises from it
        // without binning (warm_enqueue)
        int listSet = -1;
        u32 listTag = 0, listMult = 0;                   // its WarmCheck tag and cursor multiple (epoch + 1)
        bool listGated = false;                          // binned beside the raster: its plan words are the set's gplan
        // visible list: the kept pair list without the triangles that won no
        // pixel on the marking frame (a reused batch whose k_vis also set the
        // winners' bits in vmask), pruned once per generation (k_prune_list) --
        // a copy at the same offsets, so it outlives the binning set's reuse;
        // reused batches of the capturing depth mode rasterise from it
        DevArray<u32> vlist;                             // pruned pairs, tile t's vcnt[t] of them from off[t]
        DevArray<u32> vcnt;                              // ntiles kept counts | 2 check words (always 0) | the kept total
        DevArray<u32> vmask;                             // one bit per triangle: it won a pixel
        enum class VisStage { None, Marking /* marking frame enqueued */, Pruned };
        VisStage visState = VisStage::None;
        int visZ = 0;                                    // depth mode (k_vis ZMODE) of the marking frame
        int markSet = -1; u32 markTag = 0;               // the list the marking frame read (pruned from the same one)
        hipEvent_t evMark = nullptr;                     // the marking frame is done (main stream)
        // visible plan: the work items and plan words of the pruned list, planned
        // from the kept counts once per pruning (k_vis_plan, right after
        // k_prune_list) -- right-sized slices, items longest first by the
        // visible counts, no item for work the frame no longer needs
        DevArray<uint4> vitems;                          // its k_vis work items
        u32* vplan = nullptr;                            // its device totals (PW_DEV words; PW_FITS always 1)
        SeqWords hvplan;                                 // their host copy, numbered by itself (the last visible plan's)
        enum class ReplanStage { None, Enqueued, Seen /* its totals seen by the host */ };
        ReplanStage replanState = ReplanStage::None;
        BatchTotals vtotals;                             // (Seen) pairs, items, split slices, dense tiles
        u32 splitAt = 0, dslice = 0;                     // the split limits the schedule was planned under (0: defaults)
        // key cache: the final keys (zq << 32) | id of every owned tile with a kept
        // pair, as one capture frame's k_vis left them in LDS right before it shaded
        // -- a function of the buffer, the binning key and the initial depth only,
        // so later batches of the capturing mode over the same initial depth shade
        // from them (k_keys) and rasterise nothing
        DevArray<u64> kkeys;                             // TH*TW keys per cached tile, slot = the tile's item index
        DevArray<uint4> kitems;                          // an item per owned tile {tile, slot, kept pairs, 0}: cached first
        DevArray<u32> ktile;                             // the capture frame's table (KeyCaptureTable): kkeys' address, then
                                                         // per tile its slot, or ~0 (not cached)
        u32* kplan = nullptr;                            // device totals {cached tiles, items}
        SeqWords hkplan;                                 // their host copy (2 words), numbered by itself (the last key plan's)
        enum class KeyStage {
            NoMemory = -1,   // or the capture frame failed (for this generation: it stays on the visible list)
            None,
            Planned,         // item list enqueued
            Slotted,         // totals seen and slots allocated
            Capturing,       // capture frame enqueued
            Cached
        };
        KeyStage keyState = KeyStage::None;
        u32 ktiles = 0, knitems = 0;                     // (Slotted and later) cached tiles, items
        hipEvent_t evKey = nullptr;                      // the capture frame is done (main stream)
        // key index (nr_free.h KeyIndex): per cached slot the pixels' dense winner numbers, the staged winners
        // and their count, built once right after the capture frame (k_key_index; evKey covers it) -- cached
        // Gouraud batches are then shaded by k_keys_idx.  No memory: the generation stays on k_keys
        DevArray<unsigned char> kindex;                  // ktiles x (u16 idx[TH*TW]) | ktiles x (u32 win[KI_RT]) | ktiles x (u32 cnt[2])
        bool kindexed = false;                           // this generation's index is enqueued (with its capture frame)
        // key records (nr_free.h KeyRecords): the Gouraud shading record of every distinct winner of every cached
        // slot -- a function of the buffer and the binning key's transform alone.  k_key_index also leaves the
        // slots' distinct counts, a scan behind it their offsets and (hkrec) their total; once the host has seen
        // the total (no wait) the store is sized, capped (nr_key_records.h) and filled by k_key_records, and the
        // cached Gouraud batches after that one are shaded by k_keys_rec.  No memory, or over the cap: nothing
        // latched, the generation stays on k_keys_idx
        DevArray<u32> kroff;                             // ktiles distinct counts | ktiles + 1 record offsets
        DevArray<f64> krec;                              // the records (+ a tail: nr_key_records.h room_doubles)
        SeqWords hkrec;                                  // the scan's total (1 word), numbered by itself
        enum class RecStage { None, Scanned /* offsets enqueued with the index */, Ready /* records enqueued */ };
        RecStage recState = RecStage::None;
        u64 krecords = 0;                                // (Ready) records in the store
        const u32* kdist() const { return kroff.p; }
        u32* roff() const { return kroff.p + (ktiles > 1 ? ktiles : 1); }
        void drop_visible() {
            visState = VisStage::None; replanState = ReplanStage::None; keyState = KeyStage::None; kindexed = false;
            recState = RecStage::None;
        }
        void release() {
            off.release(); items.release(); off2.release();
            vlist.release(); vcnt.release(); vmask.release(); vitems.release();
            kkeys.release(); kitems.release(); ktile.release(); kindex.release();
            kroff.release(); krec.release(); hkrec.release();
            if (kplan) NR_CHECK(hipFree(kplan));
            hkplan.release();
            if (evKey) NR_CHECK(hipEventDestroy(evKey));
            if (vplan) NR_CHECK(hipFree(vplan));
            hvplan.release();
            if (evMark) NR_CHECK(hipEventDestroy(evMark));
            if (dplan) NR_CHECK(hipFree(dplan));
            if (blocks) NR_CHECK(hipFree(blocks));
            if (ready) NR_CHECK(hipEventDestroy(ready));
        }
    } sched;
    int warmMode = 0;                       // 0 automatic (NR_WARM), 1 on, 2 off (SetWarmBinning)
    u64 warmBatches = 0;                    // batches binned warm (GetWarmBatchCount)
    u64 looseBatches = 0;                   // of those, into the loose ranges (GetLooseBatchCount)
    u64 reusedBatches = 0;                  // of the warm ones, rasterised from a kept pair list (GetReusedBatchCount)
    int reuseMode = 0;                      // list reuse: 0 automatic (on), 2 off (SetListReuse)
    u64 prunedBatches = 0;                  // of the reused ones, rasterised from the visible list (GetPrunedBatchCount)
    int pruneMode = 0;                      // visible list: 0 automatic (on), 2 off (SetVisiblePruning)
    u64 replannedBatches = 0;               // of the pruned ones, rasterised under the visible plan (GetReplannedBatchCount)
    int replanMode = 0;                     // visible plan: 0 automatic (on), 2 off (SetVisibleReplan)
    u64 keyCachedBatches = 0;               // of the pruned ones, shaded from the key cache (GetKeyCachedBatchCount)
    int keyMode = 0;                        // key cache: 0 automatic (on), 2 off (SetKeyCache)
    u64 keyIndexedBatches = 0;              // of the cached ones, shaded from the key index (GetKeyIndexedBatchCount)
    int keyIndexMode = 0;                   // key index: 0 automatic (on), 2 off (SetKeyIndex)
    u64 keyRecordBatches = 0;               // of the indexed ones, shaded from the key records (GetKeyRecordBatchCount)
    int keyRecordMode = 0;                  // key records: 0 automatic (on), 2 off (SetKeyRecords)
    // Deferred stores: the record of the context's last cached batch that ran k_keys_idx.  A steady frame's f64
    // framebuffer and depth values of the cached tiles are read by nothing -- the next SetColor / ClearDepth
    // supersede them, the frame's consumer takes the frame output -- so an eligible batch (pruned_enqueue) writes
    // the frame output alone and leaves them pending here; the first use of the buffers (nr_materialize_tiles)
    // writes them, bit for bit (the KO_RESOLVE kernel over the same items, slots and index).  A batch that
    // stored its values itself leaves a record too (stored: it launches nothing), so that the rule
    // (nr_defer_policy.h) sees whether the stores were ever needed.
    // The snapshot's pointers stay those of the generation that made the record: every writer of the schedule's
    // key memory (key_plan, the capture frame, k_key_index, k_key_records, key_cache_step's regrows) sits behind frame_params,
    // which resolves the record first; so does every free but the three outside draws, which resolve
    // (DestroyTriangleBuffer) or drop (ResizeRenderContext, DestroyRenderContext) it themselves.
    struct DeferredStores {
        bool colour = false, depth = false;  // live halves (depth: a LESS + write batch only); neither: no record
        bool stored = true;                  // the batch wrote its values itself
        bool wasNeeded = false;              // a half of this record has been needed (the rule hears once)
        const TriangleBuffer* tb = nullptr;  // the buffer the snapshot's records are built from
        void* snap = nullptr;                // nrtri::DeferredSnapshot (nr_free.h), kept from record to record
        bool live() const { return colour || depth; }
    } deferred;
    nrdefer::Policy deferPolicy;
    int deferMode = 0;                      // 0 automatic (the rule), 1 always, 2 off (SetDeferredStores)
    u64 deferredBatches = 0, deferResolves = 0, deferSuperseded = 0;   // (GetDeferredStoreCounts)
    std::vector<u64> looseBanned;           // buffers whose loose binning overflowed a tile: not binned loose again
    // warm-batch checks (k_vis WarmCheck): host-mapped word a raster sets when
    // a warm batch failed them (1 binning check, 2 token timeout), read by
    // nr_settle; the batch itself was rasterised from all its triangles
    u32* hfail = nullptr; u32* dfail = nullptr;   // [0] reason, [1..3] the words it read (the message)
    u32 warmTag = 0;                        // tag of the last warm batch (k_bin_warm's error word)
    u64 warmFailures = 0;                   // warm batches that failed their checks (GetWarmFailureCount)
    std::vector<u64> warmBanned;            // buffers (uid) whose warm binning failed a check: binned cold
    int warmInject = 0;                     // testing: fault injected into the next warm batch (SetWarmFaultInjection)
    // a warm binning beside the raster was handed off by its token only (no
    // event the main stream waits on): before the main stream next writes a
    // binning set or the schedule, it waits for the binning stream (evSide)
    bool sideGated = false;
    hipEvent_t evSide = nullptr;
    void release() {
        cnt.release(); off.release(); orec.release(); tile_start.release(); tile_end.release();
        for (int k = 0; k < 2; ++k) { keys[k].release(); vals[k].release(); }
        fdone.release(); kslot.release(); stage.release(); mstage.release(); mclip.release(); mscan.release();
        minst.release();
        for (int k = 0; k < 2; ++k) {
            if (h_minst[k]) NR_CHECK(hipHostFree(h_minst[k]));
            if (evMinst[k]) NR_CHECK(hipEventDestroy(evMinst[k]));
        }
        if (temp) NR_CHECK(hipFree(temp));
        if (d_frag) NR_CHECK(hipFree(d_frag));
        if (d_flag) NR_CHECK(hipFree(d_flag));
        if (h_total) NR_CHECK(hipHostFree(h_total));
        if (hfail) NR_CHECK(hipHostFree(hfail));   // (dfail is its device address)
        if (evSide) NR_CHECK(hipEventDestroy(evSide));
        for (auto& F : fset) F.release();
        sched.release();
    }
};

enum NRKernelId { NRK_TRI_COUNT = 0, NRK_TRI_SCAN, NRK_TRI_EMIT, NRK_TRI_SORT, NRK_TILE_RANGES,
                  NRK_TILE_RASTER, NRK_PRIM, NRK_FILL, NRK_RESOLVE, NRK_VIS_INIT, NRK_OUTPUT, NRK_GATHER,
                  NRK_MESH_VERTEX, NRK_MESH_ASSEMBLE, NRK_MESH_CLIP_VERTEX, NRK_MESH_CLIP_COUNT, NRK_MESH_CLIP_SCAN,
                  NRK_MESH_CLIP_EMIT, NRK_MESH_INST_VERTEX, NRK_MESH_INST_ASSEMBLE, NRK_MESH_INST_CLIP_VERTEX,
                  NRK_MESH_INST_CLIP_COUNT, NRK_MESH_INST_CLIP_SCAN, NRK_MESH_INST_CLIP_EMIT,
                  NRK_MESH_LIGHT, NRK_MESH_LIT_ATTR, NRK_MESH_INST_LIGHT, NRK_MESH_INST_LIT_ATTR, NRK_MESH_SKIN,
                  NRK_MESH_MORPH, NRK_MESH_MORPH_SKIN, NRK_COUNT_ };

// The light state of a context's lit mesh draws (SetMeshLights; DESIGN.md §3 "Vertex lighting"): the ambient
// colour and up to MESH_MAX_LIGHTS directional lights (dx, dy, dz, cr, cg, cb), d towards the light.  51 doubles
// and a count: handed to the light kernels by value, so a draw keeps the state it was issued under.
constexpr int MESH_MAX_LIGHTS = 8;
struct MeshLights {
    f64 ambient[3] = {1, 1, 1};
    f64 light[MESH_MAX_LIGHTS][6] = {};
    int nl = 0;
};

struct RenderContext {
    i64 width = 0, height = 0;
    bool enableAlpha = false;
    f64* buffer = nullptr;            // device, row-major interleaved, W*H*ipp (cpp:3-5)
    f64 m[6] = {1, 0, 0, 1, 0, 0};    // transformMatrix (h:39)
    f64 ct[4] = {1, 1, 1, 1};         // colorTransform (h:40)
    std::vector<NRState> stack;       // stateStack (h:41)
    int device = 0;
    hipStream_t stream = nullptr;
    // depth (new)
    u32* depth = nullptr;
    bool depthTest = false, depthWrite = false;
    // deferred clears: a uniform SetColor / ClearDepth is kept pending and
    // consumed on chip by the tiled raster, or materialised before any
    // other operation that touches the buffer.
    bool pendColor = false; f64 pendColorValue = 0;
    bool pendDepth = false; u32 pendDepthValue = 0xFFFFFFFFu;
    // tile-granular pending clears (a fast clear): an order-free batch that
    // consumed a pending clear leaves the tiles no triangle touched holding it
    // in name only -- their framebuffer / depth pixels are not written; tile t
    // is such a tile while tileStamp[t] == tileEpoch (written by k_vis).  Any
    // later use of the buffers writes them first (nr_materialize_tiles), a new
    // clear of the same buffer drops them.
    bool tileColor = false; f64 tileColorValue = 0;
    bool tileDepth = false; u32 tileDepthValue = 0xFFFFFFFFu;
    u32* tileStamp = nullptr; i64 tileStampCap = 0; u32 tileEpoch = 0;
    TriScratch tri;
    // per-kernel HIP-event timing (bench.py's live roofline measurement)
    bool timing = false;
    unsigned long long timingMask = ~0ull;   // which NRKernelId are timed
    std::vector<hipEvent_t> evPool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> evPending;
    u64* tsDev = nullptr;                    // device-clock stamp pairs of timed raster launches
    std::vector<std::pair<int, int>> tsPending;   // (kernel id, pair index)
    f64 kTimeMs[NRK_COUNT_] = {0};
    i64 kCount[NRK_COUNT_] = {0};
    // covered-fragment counting (the work count of the Mpixels/s metric)
    bool countFragments = false;
    bool fragPending = false;
    u64 fragTotal = 0;
    int lastPath = 0;                 // raster of the last triangle batch (1 order-free, 2 ordered)
    int forceOrdered = 0;             // testing: always take the ordered raster
    // mesh front end (nr_mesh.hip): near plane cw = meshNear (0: off) and cull mode (0 none, 1 drops area2 > 0,
    // 2 drops area2 < 0) of this context's mesh draws -- not part of the state stack, not recorded; and the
    // triangle count the last mesh draw handed to the rasters
    f64 meshNear = 0;
    int meshCull = 0;
    bool meshPersp = false;           // textured mesh draws carry 1/cw to the rasters (SetMeshPerspective); same rule
    int texFilter = 0;                // textured triangle draws: 0 nearest, 1 bilinear (SetTriangleTextureFilter); same rule
    int texWrapU = 0, texWrapV = 0;   // their wrap addressing per axis: 0 clamp, 1 repeat, 2 mirror (SetTriangleTextureWrap); same rule
    i64 meshLastCount = 0;
    MeshLights meshLights;            // lit mesh draws (SetMeshLights): ambient (1, 1, 1), no lights; same rule
    iu8* u8buf = nullptr; size_t u8cap = 0;   // GetBufferAsUInt8 staging
    // multi-GPU: owned tile rows ty % nshards == shard (nr_dist.hip)
    int nshards = 1, shard = 0;
    // band ownership: band b belongs to rank shardPattern[b % shardPeriod]
    // (SetShard: period nshards, pattern 0..n-1; SetShardSlots: a weighted
    // interleave); every rank of a frame holds the same pattern
    int shardPeriod = 1;
    unsigned char shardPattern[64] = {0};
    // u8 frame output (GatherFrameU8, nr_dist.hip): two frame buffers, the
    // next frame renders into one while the other is assembled on the gather
    // stream; frameU8 = frameBuf[frameCur]
    iu8* frameU8 = nullptr; size_t frameU8cap = 0;
    iu8* frameBuf[2] = {nullptr, nullptr};
    int frameCur = 0, frameLast = -1;            // buffer being rendered / of the last GatherFrameU8
    iu8* stageBuf[2] = {nullptr, nullptr}; size_t stageCap[2] = {0, 0};   // packed bands per buffer
    iu8* yuvBuf = nullptr; size_t yuvCap = 0;    // GetFrameYUV420P planes (device)
    hipStream_t commStream = nullptr;            // RCCL transfers + the root's unpack
    hipEvent_t evFrameReady = nullptr, evGatherDone[2] = {nullptr, nullptr};
    hipEvent_t evDeliver[2] = {nullptr, nullptr};   // DeliverFrameU8: D2H of frame buffer x done
    bool gatherPending[2] = {false, false};
    bool frameOutput = false;   // set by GatherFrameU8: resolves also write the u8 frame
    bool frameU8Valid = false;  // frameU8 holds the u8 image of every owned pixel
    // frame output format (SetFrameFormat): 0 = the u8 image (cpp:52-57,
    // W*H*ipp bytes), 1 = its YUV420P planes (Y W*H, U and V (W/2)*(H/2);
    // W and H even), the encoder input of PutRendererContextFrame
    int frameFormat = 0;
    void* pendingBatch = nullptr;   // last visibility batch awaiting validation (nr_settle)
    // deferred command list (BeginCommandList / EndCommandList, nr_prims.hip):
    // while recording, primitive draws are queued and run together, in
    // order, by one launch (every pixel read and written once)
    bool recording = false;
    void* cmdList = nullptr;
};

struct Texture {
    i64 width = 0, height = 0;
    bool enableAlpha = false;
    f64* buffer = nullptr;            // device
    bool owns = true;                 // false: alias of a context framebuffer (cpp:377-384)
    RenderContext* aliasOf = nullptr;
    int device = 0;
};

struct TriangleBuffer {
    i64 n = 0;
    bool gouraud = false;
    f64* xy = nullptr;    // n*6   (x0,y0,x1,y1,x2,y2)
    f64* z = nullptr;     // n*3 or null
    f64* rgba = nullptr;  // n*4 (flat) or n*12 (Gouraud); null for a textured buffer
    f64* uv = nullptr;    // textured buffer (CreateTexturedTriangleBuffer): n*6 texel coordinates
    bool textured = false;
    bool opaque = false;  // every vertex alpha == 1 (known at upload; textured: decided per draw by the texture)
    int device = 0;
    // totals of the last validated binning of this buffer (nr_tri_free.hip):
    // a draw under the same key is sized from them and needs no validation
    bool known = false;
    BinKey knownKey;
    BatchTotals knownTotals;
    u64 uid = 0;          // process-unique id (a context's warm schedule names its buffer by it)
    // per cluster of CLUSTER consecutive triangles (one wave of the binning
    // kernels): its user-space bounding box {xmin, ymin, xmax, ymax} (NaN when
    // a vertex is not finite: never culled), computed at upload -- the warm
    // binning of a sharded frame skips the clusters that lie outside the
    // rank's tile rows without loading their triangles
    f64* cbox = nullptr;
    std::vector<f64> hcbox;   // (host copy: the warm schedule's active binning blocks are found on the host)
    // user-space bounding box of every vertex {xmin, ymin, xmax, ymax} (NaN: a
    // vertex is not finite): bounds how far a change of transform moves any
    // vertex on screen (loose binning, nr_tri_free.hip)
    f64 bbox[4] = {NAN, NAN, NAN, NAN};
};
constexpr int NR_CLUSTER = 64;

// host helpers shared across translation units
Texture* nr_new_texture(i64 w, i64 h, bool alpha);   // device texels, current device
// Texture source for a draw into ctx (nr_prims.hip): the texels, or -- for a
// texture that aliases ctx's own framebuffer -- a snapshot of them taken on the
// context's stream (tmp, released by nr_tex_release once the draw is enqueued).
struct TexSrc {
    const f64* ptr = nullptr;
    f64* tmp = nullptr;
};
TexSrc nr_tex_source(RenderContext* ctx, Texture* tex);
void nr_tex_release(RenderContext* ctx, TexSrc& s);
void nr_dist_sync(RenderContext* ctx);      // wait for the frame-assembly stream
u64 nr_shard_mask(const RenderContext* ctx, int rank);   // bit k: pattern slot k belongs to rank
void nr_dist_release(RenderContext* ctx);   // free the frame-output buffers
hipStream_t nr_stream_for(int device);
hipStream_t nr_bin_stream_for(int device);        // second stream: triangle binning overlapped with the raster
void nr_timing_begin_on(RenderContext* ctx, int kid, hipEvent_t* a, hipEvent_t* b, hipStream_t s);
void nr_timing_end_on(RenderContext* ctx, int kid, hipEvent_t a, hipEvent_t b, hipStream_t s);
void nr_materialize(RenderContext* ctx);          // flush pending clears
void nr_materialize_color(RenderContext* ctx);
void nr_materialize_depth(RenderContext* ctx);
void nr_materialize_tiles(RenderContext* ctx, bool color, bool depth);   // tile-granular pending clears
// deferred stores (TriScratch::DeferredStores; nr_tri_free.hip): the record's live halves among (color, depth) are
// needed -- written now if pending (nr_materialize_tiles calls it) -- or superseded by a clear; the record dropped
// with the buffers' contents (a resize), and its snapshot released; resolved in every live context whose record
// names `tb` (DestroyTriangleBuffer, nr_api.hip)
void nr_deferred_resolve(RenderContext* ctx, bool color, bool depth);
void nr_deferred_supersede(RenderContext* ctx, bool color, bool depth);
void nr_deferred_drop(RenderContext* ctx);
void nr_deferred_free(RenderContext* ctx);
void nr_deferred_resolve_buffer(const TriangleBuffer* tb);
void nr_ensure_depth(RenderContext* ctx);
void nr_timing_begin(RenderContext* ctx, int kid, hipEvent_t* a, hipEvent_t* b);
// The rasters time themselves on the device clock (FrameParams::tstamp,
// raster_stamp_begin / _end): a zeroed {start, end} pair for one timed launch,
// or null when not timed.  (Events bound to the launch, hipExtLaunchKernel
// start/stop, measured the launch gap too: profiles/r06/ab_event_every.txt.)
u64* nr_timing_stamp(RenderContext* ctx, int kid);
void nr_timing_end(RenderContext* ctx, int kid, hipEvent_t a, hipEvent_t b);
void nr_fill_f64(hipStream_t s, f64* p, i64 n, f64 v);
void nr_fill_u32(hipStream_t s, u32* p, i64 n, u32 v);
void nr_settle(RenderContext* ctx);               // validate an asynchronously sized batch, run queued commands
void nr_settle_all();                             // ... of every live context
void nr_flush_commands(RenderContext* ctx);       // run the recorded primitive draws (nr_prims.hip)
void nr_drop_commands(RenderContext* ctx);        // discard them (the whole buffer is overwritten next)
void nr_free_commands(RenderContext* ctx);        // discard and release the list storage
bool nr_record_fill(RenderContext* ctx, i64 i0, i64 i1, i64 j0, i64 j1, f64 r, f64 g, f64 b, f64 a);  // ApplyPixel over a range
bool nr_record_set_pixel(RenderContext* ctx, i64 x, i64 y, f64 r, f64 g, f64 b, f64 a);

// x86-64 cvttsd2si semantics for (i64)double: out of range / NaN -> INT64_MIN
static inline i64 nr_f2i64(f64 v) {
    if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) return LONG_MIN;
    return (i64)v;
}

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
// cpp:446-453, expression order kept: (m0*x + m2*y) + m4
__host__ __device__ __forceinline__ void nr_xform(const f64* m, f64 x, f64 y, f64& ox, f64& oy) {
    ox = m[0] * x + m[2] * y + m[4];
    oy = m[1] * x + m[3] * y + m[5];
}

// cpp:515-549 body on an already-located pixel: colour transform, then "over"
// unless a == 1; RGBA stores dst.a = a.
__device__ __forceinline__ void nr_apply_pixel(f64* p, int ipp, f64 r, f64 g, f64 b, f64 a,
                                               f64 ct0, f64 ct1, f64 ct2, f64 ct3) {
    r *= ct0; g *= ct1; b *= ct2; a *= ct3;
    if (a != 1) {
        r = p[0] * (1 - a) + r * a;
        g = p[1] * (1 - a) + g * a;
        b = p[2] * (1 - a) + b * a;
    }
    p[0] = r; p[1] = g; p[2] = b;
    if (ipp == 4) p[3] = a;
}

// cpp:555-573 nearest-texel sampler (clamp to [0,w-2]x[0,h-2]); alpha of an RGB
// texture is uninitialised in the reference (Appendix A.2) and defined as 1.
// Two inputs on which the reference is undefined are defined here (DESIGN.md §2,
// "Sampler deviations"): a NaN coordinate, which passes the
// reference's `< 0` clamp into an undefined (i64) cast, counts as 0 (the
// negated comparison below differs from `x < 0` for NaN only); and a texel
// index below 0, which only a texture 1 texel wide or high gives, reads
// texel 0.  After the clamps every coordinate lies in [-1, tw-2] x
// [-1, th-2], so both casts are defined.
__device__ __forceinline__ void nr_sample(const f64* tb, i64 tw, i64 th, bool talpha, f64 x, f64 y,
                                          f64& r, f64& g, f64& b, f64& a) {
    if (!(x >= 0)) x = 0;
    if (x >= (f64)(tw - 1)) x = (f64)(tw - 2);
    if (!(y >= 0)) y = 0;
    if (y >= (f64)(th - 1)) y = (f64)(th - 2);
    i64 ipp = talpha ? 4 : 3;
    i64 index = (i64)y * tw * ipp + (i64)x * ipp;
    if (index < 0) index = 0;   // 1-px-wide textures read index -1 in the reference (UB)
    r = tb[index + 0];
    g = tb[index + 1];
    b = tb[index + 2];
    a = talpha ? tb[index + 3] : 1.0;
}

// cpp:822-845 even-odd crossing test
template <int N>
__device__ __forceinline__ bool nr_point_in_polygon(f64 x, f64 y, const f64 (&pts)[N][2]) {
    int j = N - 1;
    bool res = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if ((pts[i][1] > y) != (pts[j][1] > y) &&
            (x < (pts[j][0] - pts[i][0]) * (y - pts[i][1]) / (pts[j][1] - pts[i][1]) + pts[i][0]))
            res = !res;
        j = i;
    }
    return res;
}

// depth quantisation (new)
__host__ __device__ __forceinline__ u32 nr_quantize_depth(f64 z) {
    if (!(z > 0.0)) return 0u;
    if (z >= 1.0) return 0xFFFFFFFFu;
    return (u32)(z * 4294967295.0);
}

// The same function without branches: clamping the product to
// [0, 4294967295] maps z <= 0 (and NaN: fmax drops it) to 0 and z >= 1 (and
// +inf) to 0xFFFFFFFF, and leaves every in-range product (hence its
// truncation) unchanged.
__device__ __forceinline__ u32 nr_quantize_depth_bl(f64 z) {
    return (u32)fmin(fmax(z * 4294967295.0, 0.0), 4294967295.0);
}

// The same function in one conversion: gfx950's v_cvt_u32_f64 truncates and
// saturates (negative and -inf to 0, >= 2^32 and +inf to 0xFFFFFFFF, NaN to
// 0), which is exactly the clamp above -- two f64 VALU operations fewer per
// fragment.  (In C++ an out-of-range cast is undefined, hence the asm.)
// Pinned against nr_quantize_depth on NaN, infinities, huge and boundary
// values by tests/test_depth_edges_gpu.py.
__device__ __forceinline__ u32 nr_quantize_depth_hw(f64 z) {
    const f64 p = z * 4294967295.0;
    u32 r;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(p));
    return r;
}

// Bytes of the context's frame output (frameFormat: u8 image or YUV420P).
static inline i64 nr_frame_bytes(const RenderContext* ctx) {
    const i64 W = ctx->width, H = ctx->height;
    return ctx->frameFormat == 1 ? W * H + 2 * (W / 2) * (H / 2) : W * H * (ctx->enableAlpha ? 4 : 3);
}

// YUV420P of the u8 image (GetFrameYUV420P, SetFrameFormat): swscale's
// unscaled RGB -> YV12 arithmetic (rgb2rgb rgb24toyv12): BT.601 limited
// range, 15-bit coefficients (0.299/0.587/0.114 x 219/255, chroma x 224/255,
// rounded), arithmetic shift, + 16 / 128; chroma point-sampled at the even
// pixel of each 2x2 block.  Parity unpinned (FFmpeg absent).
constexpr int NR_YRY = 8414, NR_YGY = 16519, NR_YBY = 3208;
constexpr int NR_YRU = -4864, NR_YGU = -9527, NR_YBU = 14392;
constexpr int NR_YRV = 14392, NR_YGV = -12060, NR_YBV = -2331;
__host__ __device__ __forceinline__ iu8 nr_y_of(int r, int g, int b) {
    return (iu8)(((NR_YRY * r + NR_YGY * g + NR_YBY * b) >> 15) + 16);
}
__host__ __device__ __forceinline__ iu8 nr_u_of(int r, int g, int b) {
    return (iu8)(((NR_YRU * r + NR_YGU * g + NR_YBU * b) >> 15) + 128);
}
__host__ __device__ __forceinline__ iu8 nr_v_of(int r, int g, int b) {
    return (iu8)(((NR_YRV * r + NR_YGV * g + NR_YBV * b) >> 15) + 128);
}

// cpp:52-57: (iu8)(v*255) = cvttsd2si to int32, keep the low byte (A.5)
__device__ __forceinline__ iu8 nr_to_u8(f64 v) {
    f64 t = v * 255;
    if (!(t > -2147483649.0 && t < 2147483648.0)) return 0;
    return (iu8)((int)t & 0xFF);
}
