// nr_free_vis.hip — the raster and shading kernels of the visibility-buffer
// raster (steps 4 and 5 of nr_tri_free.hip's head comment): k_vis, k_keys and
// the deferred shading they share.  The host reaches them through
// launch_vis_any (nr_free.h).
#include "nr_free.h"
#include "nr_tri_shade.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>

namespace nrtri {
namespace {

// Per-work-item clocks of k_vis (a build with -DNR_PROBE=1 only: tools/exp/probe.so,
// tools/exp/probe_items.py): item, {tile, list begin, end, slices}, start and end
// (s_memrealtime, 100 MHz), workgroup size.
#ifndef NR_PROBE
#define NR_PROBE 0
#endif
#if NR_PROBE
constexpr int PROBE_MAX = 65536;
__device__ unsigned long long nr_probe_buf[PROBE_MAX * 8];
__device__ unsigned int nr_probe_n;
__shared__ u64 pr_st[8];   // phase stamps of the current item (thread 0): 1 keys set, 2 raster, 3 merge, 4 hash, 5 records,
                           // 6 wave 0's first triangle data arrived, 7 wave 0's chunks done (before the barrier)
#define NR_PROBE_STAMP(k) do { if (threadIdx.x == 0) pr_st[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
__device__ __forceinline__ void probe_item(u32 item, uint4 d, u64 t0, u64 t1, int nt) {
    const u32 k = atomicAdd(&nr_probe_n, 1u);
    if (k >= PROBE_MAX) return;
    unsigned long long* e = nr_probe_buf + (size_t)k * 8;
    e[0] = (u64)item | ((u64)nt << 32);
    e[1] = (u64)d.x | ((u64)d.w << 32);
    e[2] = (u64)d.y | ((u64)d.z << 32);
    auto rel = [&](int q) { return pr_st[q] >= t0 && pr_st[q] <= t1 ? (pr_st[q] - t0) & 0xFFFF : 0xFFFFull; };
    e[4] = rel(1) | (rel(2) << 16) | (rel(3) << 32) | (rel(4) << 48);
    e[5] = rel(5) | (rel(6) << 16) | (rel(7) << 32);
    __hip_atomic_store(&e[3], (t1 - t0) | (t0 << 24), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int q = 1; q < 8; ++q) pr_st[q] = 0;
}
#else
#define NR_PROBE_STAMP(k) do { } while (0)
#endif


// k_vis occupancy: 4 waves per SIMD (<= 128 VGPRs, and LDS <= 40 KB per
// workgroup: 280 shading records over the keys + REC_EXTRA) measured 6-10 %
// faster on C3 than 3 (135 VGPRs, 53.5 KB); k_vis is latency-bound.
constexpr int VIS_WPE = 4;   // (5 waves: 96 VGPRs + 112 B spills, C3 +16 %, profiles/r05/ab_vis_occupancy.txt)

// threadIdx.x as a value the compiler cannot see through: the per-pixel LDS
// and global addresses the item phases derive from it are then formed where
// they are used, inside the item loop, instead of being hoisted to the kernel
// prologue and kept live (spilled) across the whole raster -- the 4-wave
// instances' spills were mostly those hoisted addresses.
__device__ __forceinline__ int opaque_tid() {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// ---- deferred shading --------------------------------------------------
// A workgroup shades its tile after the raster.  The winners of the tile's
// pixels are few (a triangle wins ~9 pixels of the C3 mesh), so they are
// de-duplicated in an LDS hash table, each distinct winner's data is fetched
// once (one round of independent global loads, one thread per winner) and
// turned into a shading record in LDS, and the pixels are then shaded from
// LDS.  Per-pixel dependent global loads (eight rounds of latency per
// thread) were the largest cost of the fused raster.
constexpr int REC_EXTRA = 19200;   // LDS beyond the keys for shading records (k_vis stays <= 40 KB: 4 workgroups per CU)
constexpr int HTS = 512;           // hash slots (power of two)
constexpr int HTS_WIDE = 1024;     // hash slots of the 512-thread instance (its LDS holds two workgroups per CU)
constexpr int MAXPROBE = 16;       // linear-probe limit: a winner not placed / found within it loads directly
constexpr int OVF_Q = 1;           // directly loaded records in flight per thread (0: one at a time, in pass 3)

template <int MODE, int HS = HTS>
struct ShadeStage {
    // Gouraud record: sx0 sy0 e1x e1y e2x e2y inv | c0 rgb | (c1-c0) rgb | (c2-c0) rgb
    // flat record: rgb.  Alpha is not staged: every batch routed here has
    // vertex alpha 1 (and colourTransform[3] == 1), so the interpolated alpha
    // is 1 + 0*w1 + 0*w2, computed as such.
    // LDS of a k_vis workgroup: hash table | dense-index table | keys | extra.
    // The records of the shading pass overwrite the keys (each thread keeps
    // its pixels' winners in registers by then) and run on into `extra`, so
    // a tile stages RT records in KEY_BYTES + EXTRA bytes.
    static constexpr int REC = RecLen<MODE>::REC;
    static constexpr int KEY_BYTES = TH * (TW + 1) * 8;
    static constexpr int EXTRA = MODE != ATTR_FLAT ? REC_EXTRA : 0;
    static constexpr int RT_RAW = (KEY_BYTES + EXTRA) / (REC * 8);
    static constexpr int RT = RT_RAW < TH * TW ? RT_RAW : TH * TW;   // staged records per tile
    static constexpr int HT = 0, HIDX = HS * 4, DIDX = HS * 6;
    static constexpr int KEY_OFF = ((DIDX + RT * 4) + 15) & ~15;
    static constexpr int BYTES = KEY_OFF + KEY_BYTES + EXTRA;
};

template <int HS>
__device__ __forceinline__ u32 ht_hash(u32 id) { return (id * 2654435761u) >> (32 - __builtin_ctz(HS)); }

// Dense index of winner `id` among the tile's staged records (pass 1's hash
// table), or `none` when it is not staged (its record is loaded directly).
// (The textured pass 3 uses it; the flat / Gouraud loop keeps its own inline
// probe: calling this there changes the register figures of 13 of the existing
// Gouraud k_vis instances, which are to stay as they are.)
template <int HS>
__device__ __forceinline__ int staged_record(const u32* ht, const unsigned short* hidx, u32 id, int none) {
    u32 h = ht_hash<HS>(id);
    for (int probe = 0; probe < MAXPROBE; ++probe, h = (h + 1) & (HS - 1)) {
        const u32 cur = ht[h];
        if (cur == id) return hidx[h];
        if (cur == 0) break;
    }
    return none;
}

// Shades the tile from its LDS keys (`key` at row stride KS).  Pass 1: each
// thread takes its PPT pixels (p = tid + k*NT), stores their depth, keeps
// their winners in registers and enters the distinct winners in an LDS hash
// table (dense index d).  Pass 2: one record per staged winner (independent
// global loads: one latency round), written over the keys.  Pass 3: colour,
// ApplyPixel, framebuffer (+ u8 frame) written once.  A winner past the RT
// staged records (or not placed within MAXPROBE probes) loads its own record.
// MARK (a marking frame): every pixel's winner also gets its bit in
// fp.winMask set -- here, where a winner id is read from the tile's final keys,
// so staged, overflowed and directly loaded winners are all covered (the flat
// loop per pixel; pass 1 once per distinct winner and per unstaged pixel).
__device__ __forceinline__ void mark_winner(const FrameParams& fp, u32 id) {
    __hip_atomic_fetch_or(&fp.winMask[(id - 1) >> 5], 1u << ((id - 1) & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int ZMODE, int MODEW, int NT, int HS, bool MARK = false>   // MODEW: the AttrMode, with ATTR_WRAPS for a wrapping instance
__device__ __forceinline__ void shade_tile(const FrameParams& fp, i64 x0, i64 y0, int wlim, int hlim,
                                           const u64* key, unsigned char* lds, u32& nU) {
    constexpr int MODE = attr_base(MODEW);
    constexpr bool WRAP = attr_wraps(MODEW);   // (textured instances only: the batch has a wrapped axis, fp.wrap())
    using St = ShadeStage<MODE, HS>;
    constexpr int RM = attr_unfiltered(MODE);   // the mode of the shading records (a bilinear batch: its nearest counterpart's)
    static_assert(St::REC == RecLen<RM>::REC, "the staged slots hold the records build_record<RM> writes");
    constexpr int PPT = TH * TW / NT;
    static_assert(PPT <= 32, "overflow bitmask");
    const int tid = opaque_tid();
    if constexpr (MODE == ATTR_FLAT) {
        // Flat: a winner's colour is its rgb -- no record to stage, so no
        // winner dedup: each pixel loads its winner's colour itself (the few
        // distinct winners of a tile stay in L2), FQ pixels' loads in flight
        // at a time.
        constexpr int FQ = PPT < 4 ? PPT : 4;
        static_assert(PPT % FQ == 0, "pixel groups");
#pragma unroll 1
        for (int k0 = 0; k0 < PPT; k0 += FQ) {
            u32 id[FQ];
            f64 c[FQ][3];
#pragma unroll
            for (int j = 0; j < FQ; ++j) {
                const int p = tid + (k0 + j) * NT, lx = p & (TW - 1), ly = p / TW;
                id[j] = 0;
                if (lx >= wlim || ly >= hlim) continue;
                const u64 kv = key[ly * (TW + 1) + lx];
                id[j] = (u32)kv;
                store_depth<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, kv);
                if (id[j]) {
                    if constexpr (MARK) mark_winner(fp, id[j]);
                    const f64* q = fp.src.rgba() + ((i64)id[j] - 1) * 4;
                    const double2 rg = *reinterpret_cast<const double2*>(q);
                    c[j][0] = rg.x; c[j][1] = rg.y; c[j][2] = q[2];
                }
            }
#pragma unroll
            for (int j = 0; j < FQ; ++j) {
                const int p = tid + (k0 + j) * NT, lx = p & (TW - 1), ly = p / TW;
                if (lx >= wlim || ly >= hlim) continue;
                const i64 px = x0 + lx, py = y0 + ly;
                const i64 gp = py * fp.W + px;
                if (!id[j]) {
                    if (fp.pendColor) {
                        const f64 v = fp.pendColorValue;
                        store_colour(fp, gp, px, py, v, v, v, v);
                    }
                    continue;
                }
                f64 cr = c[j][0], cg = c[j][1], cb = c[j][2], ca = 1.0;   // (record_colour's flat case)
                apply_winner(fp, gp, cr, cg, cb, ca);
                store_colour(fp, gp, px, py, cr, cg, cb, ca);
            }
        }
        return;
    }
    u32* ht = reinterpret_cast<u32*>(lds + St::HT);
    unsigned short* hidx = reinterpret_cast<unsigned short*>(lds + St::HIDX);
    u32* didx = reinterpret_cast<u32*>(lds + St::DIDX);
    f64* rec = reinterpret_cast<f64*>(lds + St::KEY_OFF);   // over the keys, after pass 1
    for (int i = tid; i < HS; i += NT) ht[i] = 0;
    if (tid == 0) nU = 0;
    __syncthreads();
    u32 ids[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) ids[k] = 0;
    // bit k: pixel k's winner is not staged -- its record is loaded directly
    // in pass 3b, OVF_Q pixels at a time.  A dense tile (more distinct
    // winners than RT, e.g. the many-sliver tiles at a mesh's poles) stops
    // inserting once RT winners are staged instead of probing a full table.
    u32 ovf = 0;
#pragma unroll 1
    for (int k = 0; k < PPT; ++k) {
        const int p = tid + k * NT, lx = p & (TW - 1), ly = p / TW;
        if (lx >= wlim || ly >= hlim) continue;
        const u64 kv = key[ly * (TW + 1) + lx];
        const u32 id = (u32)kv;
#pragma unroll
        for (int q = 0; q < PPT; ++q)
            if (q == k) ids[q] = id;   // static register index
        store_depth<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, kv);
        if (!id) continue;
        // (MARK: once per distinct winner -- by the thread that enters it in the
        // hash table -- and per pixel whose winner is not in the table)
        if (OVF_Q && __hip_atomic_load(&nU, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (u32)St::RT) {
            if constexpr (MARK) mark_winner(fp, id);
            ovf |= 1u << k;
            continue;
        }
        u32 h = ht_hash<HS>(id);
        bool placed = false;
        for (int probe = 0; probe < MAXPROBE; ++probe, h = (h + 1) & (HS - 1)) {
            const u32 cur = ht[h];
            if (cur == id) { placed = true; break; }
            if (cur == 0) {
                const u32 old = atomicCAS(&ht[h], 0u, id);
                if (old == 0) {
                    if constexpr (MARK) mark_winner(fp, id);
                    const u32 d = atomicAdd(&nU, 1u);
                    hidx[h] = (unsigned short)(d < (u32)St::RT ? d : St::RT);
                    if (d < (u32)St::RT) didx[d] = id;
                    placed = d < (u32)St::RT;
                    break;
                }
                if (old == id) { placed = true; break; }
            }
        }
        if constexpr (MARK) {
            if (!placed) mark_winner(fp, id);
        }
        if (OVF_Q && !placed) ovf |= 1u << k;
    }
    __syncthreads();   // every key read: the records may overwrite them
    NR_PROBE_STAMP(4);
    const u32 U = nU < (u32)St::RT ? nU : (u32)St::RT;
    // two winners per thread per round, both records' loads in flight
    for (u32 u = tid; u < U; u += 2 * NT) {
        RecordSrc<RM> s0, s1;
        const bool two = u + NT < U;
        load_record_src<RM>(fp, (i64)didx[u] - 1, s0);
        if (two) load_record_src<RM>(fp, (i64)didx[u + NT] - 1, s1);
        build_record<RM>(fp, s0, rec + u * St::REC);
        if (two) build_record<RM>(fp, s1, rec + (u + NT) * St::REC);
    }
    __syncthreads();
    NR_PROBE_STAMP(5);
    const TexView& tv = fp.tex;   // (textured batches)
    if constexpr (attr_textured(MODE)) {
        // Textured (any mode; the perspective record's coordinate carries the
        // divide, record_uv): a pixel's colour is a dependent gather (record -> u, v ->
        // texel, 24 B), so a thread first forms the texel offsets of TQ of its
        // pixels, then issues their loads together, and only then consumes
        // them (as the flat path keeps FQ loads in flight).  Ordinary cached
        // loads: the texture is read again by other tiles.  A bilinear mode
        // gathers four texels per pixel (24 VGPRs) and keeps the two fractions,
        // so it has one pixel's loads in flight, not two.  A modulated mode keeps
        // each pixel's record index across the gather and forms the barycentrics
        // again for the corner colours when the texel arrives (record_modulate).
        static_assert(OVF_Q > 0, "unstaged winners are shaded in pass 3b");
        constexpr bool BIL = attr_bilinear(MODE);
        constexpr bool MOD = attr_modulated(MODE);
        constexpr int TQ = BIL ? 1 : 2;
        static_assert(PPT % TQ == 0, "pixel groups");
#pragma unroll 1
        for (int k0 = 0; k0 < PPT; k0 += TQ) {
            i64 ti[TQ];   // texel offset, or -1: nothing to fetch
            f64 fu[BIL ? TQ : 1], fv[BIL ? TQ : 1];   // (bilinear: the footprint's fractions)
            int du[BIL && WRAP ? TQ : 1], dv[BIL && WRAP ? TQ : 1];   // (and under a wrap state the +1 neighbours' steps, in texels)
            int dj[MOD ? TQ : 1];                     // (modulated: the pixel's staged record)
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                const int k = k0 + j;
                ti[j] = -1;
                const int p = tid + k * NT, lx = p & (TW - 1), ly = p / TW;
                if (lx >= wlim || ly >= hlim) continue;
                const i64 px = x0 + lx, py = y0 + ly;
                u32 id = 0;
#pragma unroll
                for (int q = 0; q < PPT; ++q)
                    if (q == k) id = ids[q];
                if (!id) {
                    if (fp.pendColor) {
                        const f64 v = fp.pendColorValue;
                        store_colour(fp, py * fp.W + px, px, py, v, v, v, v);
                    }
                    continue;
                }
                if ((ovf >> k) & 1u) continue;
                const int d = staged_record<HS>(ht, hidx, id, St::RT);
                NR_DEV_CHECK(d >= St::RT || (u32)d < U,
                             "shade_tile: pixel (%ld, %ld) reads record %d of %u staged (winner %u)", (long)px, (long)py, d,
                             U, id);
                NR_DEV_CHECK(id <= (u32)fp.src.n, "shade_tile: pixel (%ld, %ld) winner %u of %ld triangles", (long)px,
                             (long)py, id, (long)fp.src.n);
                if (d >= St::RT) {
                    ovf |= 1u << k;
                    continue;
                }
                if constexpr (MOD) dj[j] = d;
                if constexpr (BIL) {
                    f64 u, v;
                    record_uv<MODE>(rec + d * St::REC, px, py, u, v);
                    if constexpr (WRAP) ti[j] = tex_bilinear_wrap(tv, fp.wrap(), u, v, fu[j], fv[j], du[j], dv[j]);
                    else ti[j] = tex_bilinear(tv, u, v, fu[j], fv[j]);
                } else {
                    if constexpr (WRAP) ti[j] = record_texel_of_wrap<MODE>(tv, fp.wrap(), rec + d * St::REC, px, py);
                    else ti[j] = record_texel_of<MODE>(tv, rec + d * St::REC, px, py);
                }
            }
            f64 c[TQ][3];
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                if (ti[j] < 0) continue;
                if constexpr (BIL) {
                    TexQuad t;
                    if constexpr (WRAP) load_tex_quad_wrap(tv, ti[j], du[j], dv[j], t);
                    else load_tex_quad(tv, ti[j], t);
                    mix_tex_quad(t, fu[j], fv[j], c[j][0], c[j][1], c[j][2]);
                } else {
                    const f64* q = tv.ptr + ti[j];
                    c[j][0] = q[0]; c[j][1] = q[1]; c[j][2] = q[2];
                }
            }
#pragma unroll
            for (int j = 0; j < TQ; ++j) {
                if (ti[j] < 0) continue;
                const int p = tid + (k0 + j) * NT, lx = p & (TW - 1), ly = p / TW;
                const i64 px = x0 + lx, py = y0 + ly;
                const i64 gp = py * fp.W + px;
                f64 cr = c[j][0], cg = c[j][1], cb = c[j][2], ca = 1.0;
                if constexpr (MOD) record_modulate(rec + dj[j] * St::REC, px, py, cr, cg, cb, ca);
                apply_winner(fp, gp, cr, cg, cb, ca);
                store_colour(fp, gp, px, py, cr, cg, cb, ca);
            }
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < PPT; ++k) {
            const int p = tid + k * NT, lx = p & (TW - 1), ly = p / TW;
            if (lx >= wlim || ly >= hlim) continue;
            const i64 px = x0 + lx, py = y0 + ly;
            const i64 gp = py * fp.W + px;
            u32 id = 0;
#pragma unroll
            for (int q = 0; q < PPT; ++q)
                if (q == k) id = ids[q];
            if (!id) {
                if (fp.pendColor) {
                    const f64 v = fp.pendColorValue;
                    store_colour(fp, gp, px, py, v, v, v, v);
                }
                continue;
            }
            if ((ovf >> k) & 1u) continue;
            int d = St::RT;
            u32 h = ht_hash<HS>(id);
            for (int probe = 0; probe < MAXPROBE; ++probe, h = (h + 1) & (HS - 1)) {
                const u32 cur = ht[h];
                if (cur == id) { d = hidx[h]; break; }
                if (cur == 0) break;
            }
            f64 cr, cg, cb, ca;
            NR_DEV_CHECK(d >= St::RT || (u32)d < U, "shade_tile: pixel (%ld, %ld) reads record %d of %u staged (winner %u)",
                         (long)px, (long)py, d, U, id);
            NR_DEV_CHECK(id <= (u32)fp.src.n, "shade_tile: pixel (%ld, %ld) winner %u of %ld triangles", (long)px, (long)py, id,
                         (long)fp.src.n);
            if (d < St::RT) {
                record_colour<MODE>(tv, rec + d * St::REC, px, py, cr, cg, cb, ca);
            } else if (OVF_Q) {
                ovf |= 1u << k;
                continue;
            } else {   // overflow: load this pixel's winner directly
                f64 r[St::REC];
                make_record<RM>(fp, (i64)id - 1, r);
                record_colour<MODE>(tv, r, px, py, cr, cg, cb, ca);
            }
            apply_winner(fp, gp, cr, cg, cb, ca);
            store_colour(fp, gp, px, py, cr, cg, cb, ca);
        }
    }
    // pass 3b: pixels whose winner is not staged, OVF_Q at a time: their
    // records' loads are independent and in flight together
    if constexpr (OVF_Q > 0) {
#pragma unroll 1
        while (ovf) {
            constexpr int Q = OVF_Q > 0 ? OVF_Q : 1;
            int kq[Q];
            RecordSrc<RM> src[Q];
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                kq[j] = -1;
                if (!ovf) continue;
                kq[j] = __builtin_ctz(ovf);
                ovf &= ovf - 1;
                u32 id = 0;
#pragma unroll
                for (int q = 0; q < PPT; ++q)
                    if (q == kq[j]) id = ids[q];
                load_record_src<RM>(fp, (i64)id - 1, src[j]);
            }
#pragma unroll
            for (int j = 0; j < Q; ++j) {
                if (kq[j] < 0) continue;
                const int p = tid + kq[j] * NT, lx = p & (TW - 1), ly = p / TW;
                const i64 px = x0 + lx, py = y0 + ly;
                const i64 gp = py * fp.W + px;
                f64 r[St::REC];
                build_record<RM>(fp, src[j], r);
                f64 cr, cg, cb, ca;
                if constexpr (WRAP) record_colour_wrap<MODE>(tv, fp.wrap(), r, px, py, cr, cg, cb, ca);
                else record_colour<MODE>(tv, r, px, py, cr, cg, cb, ca);
                apply_winner(fp, gp, cr, cg, cb, ca);
                store_colour(fp, gp, px, py, cr, cg, cb, ca);
            }
        }
    }
}

// ---- flattened chunk raster (k_vis FLAT) -------------------------------
// A wave's chunk (one triangle per lane) is rasterised in two flattened
// stages: its (triangle, row) pairs are dealt out 64 at a time (lane = row
// slot: the row's span), and each such window's covered pixels 64 at a time
// (lane = fragment) -- no lane idles on a short row or span beside a long one.
// The lanes fetch their triangle's and row's terms by lane permutes.

__device__ __forceinline__ int wave_scan_max(int v) {   // inclusive max scan (values >= 0)
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));   // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));   // row_bcast:31
    return v;
}

__device__ __forceinline__ int bperm(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
__device__ __forceinline__ u32 bperm(u32 v, int src) { return (u32)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }
__device__ __forceinline__ float bperm(float v, int src) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}
__device__ __forceinline__ f64 bperm(f64 v, int src) {
    const u64 b = __double_as_longlong(v);
    const u32 lo = (u32)__builtin_amdgcn_ds_bpermute(src << 2, (int)(u32)b);
    const u32 hi = (u32)__builtin_amdgcn_ds_bpermute(src << 2, (int)(u32)(b >> 32));
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}

// Owner of each slot of the window [wb, wb + 64) (slot wb + lane): the highest
// lane o whose run [st_o, st_o + n_o) (n_o > 0; runs in lane order, back to
// back) starts at or before it -- the runs that start in the window mark
// their first slot in the wave's 64 LDS words, an inclusive max scan carries
// each mark forward, and `carry` (the owner of slot wb - 1) fills the slots
// before the window's first mark.  (One wave, in-order LDS: the clear, the
// marks and the read need no barrier.)
__device__ __forceinline__ int window_owner(u32* mk, int lane, u32 st, u32 n, u32 wb, int carry) {
    __hip_atomic_store(&mk[lane], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (n && st - wb < 64u)
        __hip_atomic_fetch_max(&mk[st - wb], (u32)lane + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const int v = (int)__hip_atomic_load(&mk[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return max(wave_scan_max(v), carry + 1) - 1;
}

static_assert(TH <= 64, "flattened raster: a fragment's row in 6 bits");
constexpr u32 HEAVY_PRIO = 512;   // work items of at least this many triangles run at raised wave priority
constexpr int KS = TW + 1;        // padded row stride of the LDS tile keys


// One workgroup per work item (tile, slice of <= SLICE triangles).  The 4
// waves share only the tile's 2048 LDS keys; each wave independently walks
// 64-triangle chunks of the slice (chunk c goes to wave c % 4) with no
// workgroup barrier: one lane per triangle, its setup in registers (screen
// vertices, edge slopes, 1/den, depths; the next chunk's loads in flight),
// then the lane walks the triangle's rows in this tile (exact span,
// row_span_slopes) and their pixels (depth + LDS atomic on the packed key,
// two pixels per step).  Then the workgroup shades the tile (shade_tile).
// FLAT: the chunk's rows and pixels are instead dealt out 64 per window
// (flattened raster, above): for batches whose triangles cover many pixels of
// a tile (C2 -17 %, profiles/r06/ab_flat.txt); for sliver meshes the permutes
// cost more than the lane raster's idle lanes (C3 +29 %).  The host picks it
// from the previous batch's pair density (COOP_PAIRS).
// NT: workgroup size (VWG, or 2 * VWG for batches with few pairs, whose dense
// items are latency-bound: more waves per item).
// The checks of a warm batch: WarmCheck (nr_free.h).  The kernels take this
// file's own type of the same layout: their parameter types, like the kernels,
// are private to the file, which keeps every instance's symbol as it was.
struct WarmCheck : nrtri::WarmCheck {};

// One report per failed warm batch (see WarmCheck): words 1..3 for the
// message, then the reason.
__device__ __forceinline__ void warm_report(const WarmCheck& wc, u32 why, u32 a, u32 b, u32 c) {
    if (__hip_atomic_exchange(&wc.wstat[WS_REP], wc.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == wc.tag) return;
    __hip_atomic_store(&wc.hfail[1], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&wc.hfail[2], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&wc.hfail[3], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&wc.hfail[0], why, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The key cache's capture frame (KCAP instances; warm_enqueue): right before a
// workgroup shades a tile it copies the tile's final LDS keys to the tile's slot
// (tile-contiguous, rows unpadded: a wave's store is 512 contiguous bytes).
// The slots' address and the tiles' slots come from the capture table in device
// memory (fp.kcap, nr_tri.h): k_vis's arguments, and so every other instance's
// code, stay as they were.
template <int NT>
__device__ __forceinline__ void capture_keys(const KeyCaptureTable* kc, int tile, const u64* key) {
    const u32 slot = kc->slot[tile];
    if (slot == ~0u) return;
    u64* const dst = kc->keys + (size_t)slot * (TH * TW);
    const int tid = opaque_tid();
    for (int p = tid; p < TH * TW; p += NT)   // (every key: pixels past the frame edge are never shaded)
        dst[p] = key[(p / TW) * KS + (p & (TW - 1))];
}

// MARK: a marking frame's instance (shade_tile MARK; the visible list, warm_enqueue).
// KCAP: the key cache's capture frame (capture_keys at the two shade_tile calls).
template <int ZMODE, bool COUNT, int MODEW, bool FLAT, int NT, bool MARK = false, bool KCAP = false>   // ZMODE 0: no test, 1: LESS+write, 2: LESS no write
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(VIS_WPE))) void k_vis(const FrameParams fp, const uint4* __restrict__ items,
                                             const u32* __restrict__ list,
                                             u64* __restrict__ kslot, u32* __restrict__ done,
                                             const u32* __restrict__ plan, const WarmCheck wc) {
    constexpr int MODE = attr_base(MODEW);   // (the raster knows nothing of ATTR_WRAPS: only shade_tile samples)
    constexpr bool DEPTH = ZMODE != 0;
    constexpr int NWV = NT / 64;   // waves per workgroup
    // tile keys, rows padded to KS = 65 entries: lanes working on different
    // rows at the same column then hit different LDS banks
    // one LDS block (ShadeStage): hash tables | tile keys | extra; the
    // shading records overwrite the keys
    // the 512-thread instance has LDS to spare for a larger hash table (two
    // workgroups per CU)
    constexpr int HS = NT > VWG ? HTS_WIDE : HTS;
    __shared__ __attribute__((aligned(16))) unsigned char lds[ShadeStage<MODE, HS>::BYTES];
    u64* const key = reinterpret_cast<u64*>(lds + ShadeStage<MODE, HS>::KEY_OFF);
    __shared__ u32 zin[ZMODE == 2 ? TH * KS : 1];
    __shared__ u32 nU;
    __shared__ int sLast;
    __shared__ unsigned long long sFrag;
    raster_stamp_begin(fp);
    bool fb = false;   // fallback: every triangle of the batch against every tile (WarmCheck)
    if (wc.wstat) {
        const u32 wt = __hip_atomic_load(&wc.wstat[WS_TAG], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fb = !plan[PW_FITS] || wt == wc.tag;
        if (fb && blockIdx.x == 0 && threadIdx.x == 0) warm_report(wc, plan[PW_FITS] ? 1u : 2u, ~0u, wt, wc.tag);
    } else if (!plan[PW_FITS]) {
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: the chunk loop is a scalar loop)
    const u32 nitems = plan[PW_ITEMS];
    unsigned long long myFrags = 0;
    if (COUNT && tid == 0) sFrag = 0;
    // grid-stride over the work items (the grid is sized from a capacity
    // bound, not from the item count, so no host sync is needed)
    uint4 dnext = blockIdx.x < nitems ? items[blockIdx.x] : make_uint4(0, 0, 0, 0);
    u32 badTile = ~0u;   // a tile of this workgroup's whose cursor check failed (WarmCheck)
#if NR_PROBE
    u64 pr_t0 = 0;
    u32 pr_item = ~0u;
    uint4 pr_d = make_uint4(0, 0, 0, 0);
#endif
    for (u32 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const uint4 d = dnext;
        if (item + gridDim.x < nitems) dnext = items[item + gridDim.x];
#if NR_PROBE
        if (tid == 0) {
            const u64 now = __builtin_amdgcn_s_memrealtime();
            if (pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, now, NT);
            pr_t0 = now; pr_item = item; pr_d = d;
        }
#endif
        __syncthreads();
        const int itid = opaque_tid();   // (this item's per-pixel addresses: formed here, not kept live)
        const int tile = (int)d.x;
        u32 ls = d.y, le = d.z;
        const u32 nsl = d.w & 0xFFFFu;   // slices of the tile (d.w >> 16: this item's slice)
        const bool multi = nsl > 1;
        bool fbt = fb;   // this tile's list is not trusted (WarmCheck)
        if (wc.wstat && !fb) {
            // (uniform values: scalar registers, nothing kept in VGPRs across the item)
            const u32 beg = __builtin_amdgcn_readfirstlane(wc.off[tile]);
            const u32 cnt = __builtin_amdgcn_readfirstlane(wc.off[tile + 1]) - beg;
            const u32 cu = __builtin_amdgcn_readfirstlane(
                __hip_atomic_load(&wc.cur[tile], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (!wc.loose) {
                fbt = cu != wc.mult * cnt;
            } else {
                fbt = cu > cnt;
                if (!fbt) {   // this item's slice of the tile's cu pairs
                    const u32 k = d.w >> 16;
                    ls = beg + (u32)(((u64)k * cu) / nsl);
                    le = beg + (u32)(((u64)(k + 1) * cu) / nsl);
                }
            }
            if (fbt) badTile = (u32)tile;   // (reported after the item loop: no report code live in it)
        }
        if (fbt) {   // this item's slice of all n triangles (never empty: a split tile has n >= its pairs > nsl)
            const u64 n = (u64)fp.src.n, k = d.w >> 16;
            ls = (u32)(k * n / nsl);
            le = (u32)((k + 1) * n / nsl);
        }
        constexpr int rlo = 0;
        // the longest work items (dense tiles' slices, and the slices of split
        // tiles, whose last slice merges and shades: the longest chains) set
        // the kernel's critical path: their waves win the SIMD's issue
        // arbitration over the short items that run beside them
        if (le - ls >= HEAVY_PRIO || multi) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(0);
        const int tx = tile % fp.tiles_x, ty = tile / fp.tiles_x;
        const i64 x0 = (i64)tx * TW, y0 = (i64)ty * TH;
        const int wlim = (int)(fp.W - x0 < TW ? fp.W - x0 : TW);
        const int hlim = (int)(fp.H - y0 < TH ? fp.H - y0 : TH);
        const int rcap = hlim;   // rows [rlo, rcap) of the tile are rasterised here
        if (ls == le && !multi) {   // no triangle: only the pending clears
            if (fp.tileStamp) {
                // fast clear: the tile's framebuffer and depth keep the clear
                // pending (RenderContext::tileStamp); only the frame output,
                // which the batch hands over, is written
                if (fp.frameU8 && fp.pendColor) {
                    const f64 v = fp.pendColorValue;
                    for (int p = itid; p < TH * TW; p += NT) {
                        const int lx = p & (TW - 1), ly = p / TW;
                        if (lx < wlim && ly < hlim)
                            store_frame_out(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly, v, v, v, v);
                    }
                }
                if (itid == 0) fp.tileStamp[tile] = fp.tileEpoch;
                continue;
            }
            for (int p = itid; p < TH * TW; p += NT) {
                const int lx = p & (TW - 1), ly = p / TW;
                if (lx < wlim && ly < hlim)
                    store_clear<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly);
            }
            continue;
        }

        for (int p = itid; p < TH * TW; p += NT) {
            const int lx = p & (TW - 1), ly = p / TW;
            u32 z0 = 0xFFFFFFFFu;
            if (DEPTH && lx < wlim && ly < hlim)
                z0 = fp.pendDepth ? fp.pendDepthValue : fp.depth[(y0 + ly) * fp.W + x0 + lx];
            key[ly * KS + lx] = ZMODE == 1 ? ((u64)z0 << 32) : 0ull;
            if (ZMODE == 2) zin[ly * KS + lx] = z0;
        }
        __syncthreads();
        NR_PROBE_STAMP(1);

        // this wave's chunks: c = wave, wave + NW, ...  One lane per triangle,
        // its setup in registers; the lane walks the triangle's rows in this
        // tile (exact span from the per-edge slopes) and their pixels -- or,
        // FLAT, the chunk's rows and then their pixels are dealt out to the
        // lanes 64 per window.  A short slice is cut into NW chunks so that
        // every wave gets a share.
        const u32 ns = le - ls;
        const u32 cs = ns >= 64u * NWV ? 64u : (ns + NWV - 1) / NWV;
        const u32 nch = (ns + cs - 1) / cs;
        // Loads run two chunks ahead for the list and one chunk ahead for the
        // triangle data: chunk c's setup issues the vertex loads of chunk
        // c + NWV from an index that arrived during chunk c - NWV, and the
        // index of chunk c + 2 NWV -- the dependent list -> vertex load pair
        // is never waited on inside a chunk (it used to stall every chunk
        // for one memory latency before the setup).
        // Every load here is unconditional, from an in-range address (a lane
        // past the chunk reads the slice's first entry, a real triangle), and
        // nothing is computed from a loaded value until it is used: a
        // conditional load, or a use right after it, makes the compiler wait
        // for the loads in flight on the spot.
        auto list_at = [&](u32 c) -> u32 {
            const int ln = opaque_tid() & 63;   // (formed here: the lane index is not kept live across the item)
            const u32 b = ls + c * cs + ln;
            const u32 i = c < nch && (u32)ln < cs && b < le ? b : ls;
            return fbt ? i : list[i];   // (fallback: the slice's triangle ids themselves)
        };
        // chunk c + NWV's triangle (loaded) and chunk c + 2 NWV's (in flight)
        u32 pt = list_at(wave), ptn = list_at(wave + NWV);
        const bool hasZ = DEPTH && fp.src.z;
        const f64* const zsrc = hasZ ? fp.src.z : fp.src.xy;   // (no z: any valid address, values unused)
        f64 pxy[6], pz[3];
        auto prefetch = [&](u32 t) {
            load_tri_xy(fp.src.xy, t, pxy);
            if (DEPTH) {
                const f64* qz = zsrc + (i64)t * 3;
                pz[0] = qz[0]; pz[1] = qz[1]; pz[2] = qz[2];
            }
        };
        // (FLAT: the chunk's vertices are loaded at its start -- a flattened
        // chunk runs long enough that its next one's loads would only hold
        // registers through it)
        if (!FLAT) prefetch(pt);
        for (u32 c = wave; c < nch; c += NWV) {
            const u32 base = ls + c * cs;
            const int cnt = (int)((le - base) < cs ? (le - base) : cs);
            if (FLAT) prefetch(pt);
            const u32 t = pt;
            f64 sx[3], sy[3], sl[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) nr_xform(fp.m, pxy[2 * v], pxy[2 * v + 1], sx[v], sy[v]);
#if NR_PROBE
            if (threadIdx.x == 0 && c == (u32)wave) pr_st[6] = __builtin_amdgcn_s_memrealtime() + (sx[0] != sx[0] ? 1 : 0);
#endif
            const f64 zz0 = hasZ ? pz[0] : 0.0;
            const f64 dz1 = hasZ ? pz[1] - pz[0] : 0.0, dz2 = hasZ ? pz[2] - pz[0] : 0.0;
            pt = ptn;
            if (!FLAT) prefetch(pt);
            ptn = list_at(c + 2 * NWV);
            const f64 e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
            const f64 den = e1x * e2y - e2x * e1y;
            int r0 = 0, r1 = 0;   // rows with a straddling edge: ymin <= y < ymax (exact)
            if (lane < cnt && tri_finite(sx, sy) && den != 0) {
                const f64 ymn = fmin(fmin(sy[0], sy[1]), sy[2]), ymx = fmax(fmax(sy[0], sy[1]), sy[2]);
                r0 = (int)clampd(ceil(ymn) - (f64)y0, (f64)rlo, (f64)rcap);
                r1 = (int)clampd(ceil(ymx) - (f64)y0, (f64)rlo, (f64)rcap);
            }
            edge_slopes(sx, sy, sl);
            const f64 inv = 1.0 / den;
            const u64 id1 = (u64)t + 1;
            // f32 row spans (row_span32) with the exact f64 row_span_in for the
            // rows the f32 bound cannot decide: C2 -2 %, one rank's 8-way C3
            // share -3 % (k_vis 44 -> 40 us; profiles/r03_c3/ab_span32.txt).
            // Flat batches keep the f64 spans (the f32 ones cost the flat
            // instances 8-24 B/lane of spills), and so do textured batches in
            // the lane raster (with the f32 spans its LESS + write instances
            // need 12 B/lane of scratch; with the f64 ones 119 VGPRs, none).
            constexpr bool SPAN32 = (MODE == ATTR_GOURAUD || (attr_textured(MODE) && FLAT)) && ZMODE != 2 && !COUNT;
            if constexpr (FLAT) {
                // rows: the chunk's (triangle, row) pairs, 64 per window
                const u32 nr = r0 < r1 ? (u32)(r1 - r0) : 0u;
                const u32 rin = wave_scan(nr, lane);
                const u32 R = (u32)__builtin_amdgcn_readlane((int)rin, 63), rex = rin - nr;
                const int r0x = r0 - (int)rex;   // (row of slot s: s + r0x of its triangle's lane)
                Span32 S32;
                if (SPAN32) S32 = span32_setup(sx, sy, sl, (f64)x0, (f64)y0);
                u32* const mk = reinterpret_cast<u32*>(lds + ShadeStage<MODE, HS>::HT) + wave * 64;
                int rcar = -1;
                for (u32 rb = 0; rb < R; rb += 64) {
                    const int o = window_owner(mk, lane, rex, nr, rb, rcar);
                    rcar = __builtin_amdgcn_readlane(o, 63);
                    const u32 slot = rb + (u32)lane;
                    const int r = (int)slot + bperm(r0x, o);
                    const f64 y = (f64)(int)(y0 + r);
                    // (every permute with all lanes active: a permute reads 0 from an inactive lane)
                    Span32 S;
                    f64 ox[3], oy[3], os[3];
                    u32 oid = 0;
                    if (SPAN32) {
                        S.L = {bperm(S32.L.x, o), bperm(S32.L.yhi, o), bperm(S32.L.ylo, o), bperm(S32.L.s, o),
                               bperm(S32.L.ce, o)};
                        S.T = {bperm(S32.T.x, o), bperm(S32.T.yhi, o), bperm(S32.T.ylo, o), bperm(S32.T.s, o),
                               bperm(S32.T.ce, o)};
                        S.B = {bperm(S32.B.x, o), bperm(S32.B.yhi, o), bperm(S32.B.ylo, o), bperm(S32.B.s, o),
                               bperm(S32.B.ce, o)};
                        S.ymid = bperm(S32.ymid, o);
                        oid = bperm((u32)id1, o);
                    } else {
#pragma unroll
                        for (int v = 0; v < 3; ++v) {
                            ox[v] = bperm(sx[v], o); oy[v] = bperm(sy[v], o); os[v] = bperm(sl[v], o);
                        }
                    }
                    int xs = 0, xe = 0;
                    if (slot < R) {
                        if (SPAN32) {
                            if (!row_span32(S, r, y, (float)wlim, xs, xe)) {
                                f64 qx[3], qy[3];
                                tri_screen(fp.src, fp.m, (i64)oid - 1, qx, qy);
                                row_span_in(qx, qy, y, (f64)x0, (f64)wlim, xs, xe);
                            }
                        } else {
                            row_span_slopes(ox, oy, os, y, (f64)x0, (f64)wlim, xs, xe);
                        }
                    }
                    if (COUNT) myFrags += (unsigned long long)(xe - xs);
                    const u32 len = xe > xs ? (u32)(xe - xs) : 0u;
                    // the row's depth terms (frag_depth's e2x * dy and e1x * dy) and its
                    // triangle's, held by the row's lane: a fragment fetches all of its
                    // terms from one lane (one permute round)
                    f64 t1 = 0.0, t2 = 0.0, ox0 = 0.0, oe1y = 0.0, oe2y = 0.0, oin = 0.0, oz0 = 0.0, od1 = 0.0, od2 = 0.0;
                    const u32 rid = bperm((u32)id1, o);
                    if (ZMODE != 0) {
                        const f64 dy = y - bperm(sy[0], o);
                        t1 = bperm(e2x, o) * dy;
                        t2 = bperm(e1x, o) * dy;
                        ox0 = bperm(sx[0], o); oe1y = bperm(e1y, o); oe2y = bperm(e2y, o);
                        oin = bperm(inv, o); oz0 = bperm(zz0, o); od1 = bperm(dz1, o); od2 = bperm(dz2, o);
                    }
                    // fragments of the window's rows, 64 per step
                    const u32 fin = wave_scan(len, lane);
                    const u32 F = (u32)__builtin_amdgcn_readlane((int)fin, 63), fex = fin - len;
                    const int pk = (xs - (int)fex) * 64 + r;   // x - f, row
                    int fcar = -1;
                    for (u32 f0 = 0; f0 < F; f0 += 64) {
                        const int q = window_owner(mk, lane, fex, len, f0, fcar);
                        fcar = __builtin_amdgcn_readlane(q, 63);
                        const int pq = bperm(pk, q);
                        const u32 fid = bperm(rid, q);
                        const int rr = pq & 63;
                        const int xx = (int)(f0 + (u32)lane) + (pq >> 6);
                        if (ZMODE == 0) {
                            if (f0 + (u32)lane < F) atomicMax(&key[rr * KS + xx], (u64)fid);
                            continue;
                        }
                        const f64 T1 = bperm(t1, q), T2 = bperm(t2, q);
                        const f64 qx0 = bperm(ox0, q), qe1y = bperm(oe1y, q), qe2y = bperm(oe2y, q);
                        const f64 qin = bperm(oin, q), qz0 = bperm(oz0, q), qd1 = bperm(od1, q), qd2 = bperm(od2, q);
                        if (f0 + (u32)lane < F) {
                            // frag_depth with the row's products: the same operations on the same values
                            const f64 X = (f64)(int)(x0 + xx);
                            const f64 dx = X - qx0;
                            const f64 w1 = (dx * qe2y - T1) * qin;
                            const f64 w2 = (T2 - dx * qe1y) * qin;
                            const f64 zz = qz0 + qd1 * w1 + qd2 * w2;
                            const u32 zq = nr_quantize_depth_hw(zz);
                            const int kp = rr * KS + xx;
                            if (ZMODE == 1) atomicMin(&key[kp], ((u64)zq << 32) | fid);
                            else if (zq < zin[kp]) atomicMax(&key[kp], (u64)fid);
                        }
                    }
                }
                continue;
            }
            if (r0 < r1) {
                Span32 S32;
                if (SPAN32) S32 = span32_setup(sx, sy, sl, (f64)x0, (f64)y0);
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                for (int r = r0; r < r1; ++r) {
                    const f64 y = (f64)(int)(y0 + r);
                    int xs, xe;
                    if (!SPAN32) {
                        row_span_slopes(sx, sy, sl, y, (f64)x0, (f64)wlim, xs, xe);
                    } else if (!row_span32(S32, r, y, (float)wlim, xs, xe)) {
                        // (rare: the exact statement.)  The screen vertices are
                        // formed again from the triangle's positions rather than
                        // kept live through the row loop: 8 fewer VGPRs there,
                        // the 4-wave instances' register peak
                        f64 qx[3], qy[3];
                        tri_screen(fp.src, fp.m, (i64)id1 - 1, qx, qy);
                        row_span_in(qx, qy, y, (f64)x0, (f64)wlim, xs, xe);
                    }
                    if (COUNT) myFrags += (unsigned long long)(xe - xs);
                    if (xs >= xe) continue;
                    if (ZMODE == 0) {
#pragma clang loop vectorize(disable) interleave(disable)
                        for (int lx = xs; lx < xe; ++lx) atomicMax(&key[r * KS + lx], id1);
                        continue;
                    }
                    const f64 dy = y - sy[0];   // (f64)j - pts[0][1], as the oracle
                    // two pixels per step: independent chains (ILP) and half the
                    // divergent trip count for the short spans of sliver triangles
                    f64 X = (f64)(int)(x0 + xs);   // pixel x as f64, exact (integers < 2^31)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                    for (int lx = xs; lx < xe; lx += 2, X += 2.0) {
                        frag_key<ZMODE>(key, zin, r * KS + lx, X, dy, sx[0], e1x, e1y, e2x, e2y, inv, zz0, dz1, dz2,
                                        id1);
                        if (lx + 1 < xe)
                            frag_key<ZMODE>(key, zin, r * KS + lx + 1, X + 1.0, dy, sx[0], e1x, e1y, e2x, e2y, inv,
                                            zz0, dz1, dz2, id1);
                    }
                }
            }
        }
        NR_PROBE_STAMP(7);
        __syncthreads();
        NR_PROBE_STAMP(2);
        if (!multi) {   // the whole list was in this slice: shade now
            if constexpr (KCAP) capture_keys<NT>(fp.kcap, tile, key);
            if (rlo < rcap)
                shade_tile<ZMODE, MODEW, NT, HS, MARK>(fp, x0, y0 + rlo, wlim, rcap - rlo, key + rlo * KS, lds, nU);
            continue;
        }
        // split tile (a dense tile's slice): the slice's keys go to its own
        // slot of `kslot` (slot = item index: the split tiles' items come first
        // in the item list, plan kernels), as plain agent-coherent stores -- no
        // read-modify-write, so the slices of a tile never contend; the slice
        // that finishes last reduces every slot of the tile (min for LESS +
        // write, max of the ids otherwise: every slot starts from the same
        // initial keys) into its LDS keys and shades the tile.  The hand-off
        // needs no cache-wide fence: the slots move through agent-scope
        // (sc1) stores and loads, each wave drains its stores before the
        // barrier, and the slice counter is a relaxed device atomic.
        {
            u64* const mine = kslot + (size_t)item * (TH * TW);
            for (int p = itid; p < TH * TW; p += NT)   // (every key: pixels past the frame edge are never shaded)
                __hip_atomic_store(&mine[p], key[(p / TW) * KS + (p & (TW - 1))], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_s_waitcnt(0);   // vmcnt = lgkmcnt = 0: this wave's stores performed
        __syncthreads();
        if (tid == 0) {
            const u32 prev = __hip_atomic_fetch_add(&done[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sLast = prev + 1 == nsl;
            if (prev + 1 == nsl) __hip_atomic_store(&done[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!sLast) continue;
        {
            // each thread reduces its PR pixels together: per slot, PR
            // independent loads in flight (one latency round per slot, not
            // per pixel and slot)
            const u32 first = item - (d.w >> 16);   // the tile's first slice (its slot)
            constexpr int PR = TH * TW / NT;
            u64 kk[PR];
#pragma unroll
            for (int j = 0; j < PR; ++j) {
                const int p = itid + j * NT;
                kk[j] = key[(p / TW) * KS + (p & (TW - 1))];
            }
            // MB slots per round, all their loads in flight together (16 keys
            // per thread): a 16-slice pole tile's merge is 4 latency rounds,
            // not 16.  This slice's own slot and the padding past the last
            // slice read slot `first` again: min / max are idempotent.
            constexpr int MB = PR >= 8 ? 2 : (PR >= 4 ? 4 : 8);
            for (u32 sl = 0; sl < nsl; sl += MB) {
                u64 v[MB][PR];
#pragma unroll
                for (int b = 0; b < MB; ++b) {
                    const u32 s2 = sl + b < nsl ? sl + b : 0u;
                    const u64* slot = kslot + (size_t)(first + s2) * (TH * TW);
#pragma unroll
                    for (int j = 0; j < PR; ++j)
                        v[b][j] = __hip_atomic_load(slot + itid + j * NT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
#pragma unroll
                for (int b = 0; b < MB; ++b)
#pragma unroll
                    for (int j = 0; j < PR; ++j)
                        kk[j] = ZMODE == 1 ? (v[b][j] < kk[j] ? v[b][j] : kk[j]) : (v[b][j] > kk[j] ? v[b][j] : kk[j]);
            }
#pragma unroll
            for (int j = 0; j < PR; ++j) {
                const int p = itid + j * NT;
                key[(p / TW) * KS + (p & (TW - 1))] = kk[j];
            }
        }
        __syncthreads();
        NR_PROBE_STAMP(3);
        if constexpr (KCAP) capture_keys<NT>(fp.kcap, tile, key);
        shade_tile<ZMODE, MODEW, NT, HS, MARK>(fp, x0, y0, wlim, hlim, key, lds, nU);
    }   // work items
#if NR_PROBE
    if (tid == 0 && pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, __builtin_amdgcn_s_memrealtime(), NT);
#endif
    raster_stamp_end(fp);
    if (badTile != ~0u && tid == 0)
        warm_report(wc, wc.loose ? 4u : 3u, badTile, wc.cur[badTile],
                    (wc.loose ? 1u : wc.mult) * (wc.off[badTile + 1] - wc.off[badTile]));
    if (COUNT) {
        __syncthreads();
        atomicAdd(&sFrag, myFrags);
        __syncthreads();
        if (tid == 0) atomicAdd(fp.fragCounter, sFrag);
    }
}

// ---- key cache: the steady kernel ---------------------------------------------
// An unchanged draw's final keys are the same every frame (same buffer, same
// binning key, same initial depth: the conditions of a marking frame), so once
// a capture frame has stored them (k_vis KCAP) a batch needs none of k_vis's key
// pass -- no key set-up, no list or vertex loads, no f64 triangle set-up, no LDS
// atomics.  One workgroup per owned tile (grid-strided over the key items,
// k_key_plan): an empty item takes k_vis's empty-tile path; a cached one loads
// its 2048 keys (every load of a thread in flight together, a wave's load 512
// contiguous bytes), stores them to the LDS keys at stride KS and shades the
// tile with shade_tile unchanged -- everything colour-side is read live from fp.
// kplan: {cached tiles, items}.
template <int ZMODE, int MODEW, int NT>
__global__ __launch_bounds__(NT) void k_keys(const FrameParams fp, const uint4* __restrict__ items,
                                             const u64* __restrict__ kkeys, const u32* __restrict__ kplan) {
    constexpr int MODE = attr_base(MODEW);
    constexpr int HS = NT > VWG ? HTS_WIDE : HTS;
    constexpr int PPT = TH * TW / NT;
    __shared__ __attribute__((aligned(16))) unsigned char lds[ShadeStage<MODE, HS>::BYTES];
    u64* const key = reinterpret_cast<u64*>(lds + ShadeStage<MODE, HS>::KEY_OFF);
    __shared__ u32 nU;
    raster_stamp_begin(fp);
    const u32 nitems = kplan[1];
    uint4 dnext = blockIdx.x < nitems ? items[blockIdx.x] : make_uint4(0, 0, 0, 0);
#if NR_PROBE
    const int tid = threadIdx.x;
    u64 pr_t0 = 0;
    u32 pr_item = ~0u;
    uint4 pr_d = make_uint4(0, 0, 0, 0);
#endif
    for (u32 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const uint4 d = dnext;
        if (item + gridDim.x < nitems) dnext = items[item + gridDim.x];
#if NR_PROBE
        if (tid == 0) {   // (the record's list range: [0, kept pairs))
            const u64 now = __builtin_amdgcn_s_memrealtime();
            if (pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, now, NT);
            pr_t0 = now; pr_item = item; pr_d = make_uint4(d.x, 0u, d.z, 1u);
        }
#endif
        __syncthreads();   // (the last item's records lie over the keys)
        const int itid = opaque_tid();
        const int tile = (int)d.x;
        const int tx = tile % fp.tiles_x, ty = tile / fp.tiles_x;
        const i64 x0 = (i64)tx * TW, y0 = (i64)ty * TH;
        const int wlim = (int)(fp.W - x0 < TW ? fp.W - x0 : TW);
        const int hlim = (int)(fp.H - y0 < TH ? fp.H - y0 : TH);
        if (d.y == ~0u) {   // no kept pair: only the pending clears (as k_vis)
            if (fp.tileStamp) {
                if (fp.frameU8 && fp.pendColor) {
                    const f64 v = fp.pendColorValue;
                    for (int p = itid; p < TH * TW; p += NT) {
                        const int lx = p & (TW - 1), ly = p / TW;
                        if (lx < wlim && ly < hlim)
                            store_frame_out(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly, v, v, v, v);
                    }
                }
                if (itid == 0) fp.tileStamp[tile] = fp.tileEpoch;
                continue;
            }
            for (int p = itid; p < TH * TW; p += NT) {
                const int lx = p & (TW - 1), ly = p / TW;
                if (lx < wlim && ly < hlim)
                    store_clear<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly);
            }
            continue;
        }
        const u64* const src = kkeys + (size_t)d.y * (TH * TW);
        u64 kv[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) kv[k] = src[itid + k * NT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = itid + k * NT;
            key[(p / TW) * KS + (p & (TW - 1))] = kv[k];
        }
        __syncthreads();
        NR_PROBE_STAMP(1);
        NR_PROBE_STAMP(2);
        shade_tile<ZMODE, MODEW, NT, HS>(fp, x0, y0, wlim, hlim, key, lds, nU);
    }
#if NR_PROBE
    if (tid == 0 && pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, __builtin_amdgcn_s_memrealtime(), NT);
#endif
    raster_stamp_end(fp);
}

// ---- key index ----------------------------------------------------------------
// What shade_tile's pass 1 finds out about a tile -- its distinct winners, a
// dense number for each -- depends on the tile's keys alone, and a key cache's
// keys never change.  k_key_index finds it once per generation, right after the
// capture frame (one 256-thread workgroup per cached slot), and k_keys_idx then
// shades a cached Gouraud tile without a hash table: keys and index entries
// loaded together, depths stored from the keys in registers, one record per
// staged winner (ids from the slot's winner list), one barrier, and every pixel
// reads its record by the dense number the index gives it.
//
// The build is deterministic: the winners are numbered by their first pixel in
// p order (p = ly * TW + lx), so the staged ones of a tile with more than KI_RT
// are those whose first pixel comes first.  The table has two slots per pixel
// and is probed without a limit, so cnt is exactly min(distinct, KI_RT).  Every
// pixel's entry is its winner's true dense number, staged or not (a number from
// KI_RT on is what k_keys_idx takes as "not staged", and where k_keys_rec finds
// the record in the slot's part of the record store); kdist, when given, gets
// the uncapped distinct count (the record scan's input).
constexpr int KI_HS = 2 * TH * TW;   // hash slots of k_key_index (power of two)
constexpr int KI_NT = 256;           // its workgroup: thread t numbers pixels [t * KI_PPT, (t + 1) * KI_PPT)
constexpr int KI_PPT = TH * TW / KI_NT;
static_assert(TH * TW < KI_DIRECT, "a dense number fits the index entry");

__global__ __launch_bounds__(KI_NT) void k_key_index(const uint4* __restrict__ items, const u64* __restrict__ kkeys,
                                                     u32 tiles, unsigned short* __restrict__ kidx, u32* __restrict__ kwin,
                                                     u32* __restrict__ kcnt, u32* __restrict__ kdist, i64 W, i64 H,
                                                     int tiles_x) {
    __shared__ u32 ht[KI_HS];               // winner ids (0: free)
    __shared__ u32 hfirst[KI_HS];           // per table slot: the winner's first pixel
    __shared__ unsigned short hd[KI_HS];    // ... and then its dense number
    __shared__ u32 scan[KI_NT];
    __shared__ u32 nDirect;
    const u32 slot = blockIdx.x;
    if (slot >= tiles) return;
    const int tid = threadIdx.x;
    const int tile = (int)items[slot].x;    // (a cached item's slot is its index, k_key_plan)
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const i64 x0 = (i64)tx * TW, y0 = (i64)ty * TH;
    const int wlim = (int)(W - x0 < TW ? W - x0 : TW);
    const int hlim = (int)(H - y0 < TH ? H - y0 : TH);
    for (int i = tid; i < KI_HS; i += KI_NT) { ht[i] = 0; hfirst[i] = ~0u; }
    if (tid == 0) nDirect = 0;
    __syncthreads();
    const u64* const src = kkeys + (size_t)slot * (TH * TW);
    u32 id[KI_PPT], hs[KI_PPT];
#pragma unroll
    for (int k = 0; k < KI_PPT; ++k) {
        const int p = tid * KI_PPT + k, lx = p & (TW - 1), ly = p / TW;
        id[k] = lx < wlim && ly < hlim ? (u32)src[p] : 0u;
        hs[k] = 0;
        if (!id[k]) continue;
        u32 h = (id[k] * 2654435761u) >> (32 - __builtin_ctz(KI_HS));
        for (;; h = (h + 1) & (KI_HS - 1)) {   // (ends: at most TH * TW ids in twice as many slots)
            const u32 cur = ht[h];
            if (cur == id[k]) break;
            if (cur == 0) {
                const u32 old = atomicCAS(&ht[h], 0u, id[k]);
                if (old == 0 || old == id[k]) break;
            }
        }
        hs[k] = h;
        atomicMin(&hfirst[h], (u32)p);
    }
    __syncthreads();
    // the winners' dense numbers: the rank of their first pixels
    u32 mine = 0;
#pragma unroll
    for (int k = 0; k < KI_PPT; ++k)
        if (id[k] && hfirst[hs[k]] == (u32)(tid * KI_PPT + k)) ++mine;
    scan[tid] = mine;
    __syncthreads();
    for (int o = 1; o < KI_NT; o <<= 1) {   // inclusive scan
        const u32 v = tid >= o ? scan[tid - o] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    u32 d = scan[tid] - mine;
    const u32 distinct = scan[KI_NT - 1];
#pragma unroll
    for (int k = 0; k < KI_PPT; ++k) {
        if (!id[k] || hfirst[hs[k]] != (u32)(tid * KI_PPT + k)) continue;
        hd[hs[k]] = (unsigned short)d;
        if (d < (u32)KI_RT) kwin[(size_t)slot * KI_RT + d] = id[k];
        ++d;
    }
    __syncthreads();
    u32 direct = 0;
#pragma unroll
    for (int k = 0; k < KI_PPT; ++k) {
        unsigned short v = KI_NONE;
        if (id[k]) {
            v = hd[hs[k]];
            if (v >= KI_RT) ++direct;
        }
        kidx[(size_t)slot * (TH * TW) + tid * KI_PPT + k] = v;
    }
    if (direct) atomicAdd(&nDirect, direct);
    __syncthreads();
    if (tid == 0) {
        kcnt[2 * (size_t)slot] = distinct < (u32)KI_RT ? distinct : (u32)KI_RT;
        kcnt[2 * (size_t)slot + 1] = nDirect;
        if (kdist) kdist[slot] = distinct;
    }
}

// ---- key records --------------------------------------------------------------
// The record offsets of the cached slots: roff[s] = the distinct winners of the
// slots before s, roff[tiles] their total, which also goes to the host under
// seq (SeqWords).  One workgroup: thread t sums a contiguous run of slots.
constexpr int KR_SCAN_NT = 256;
__global__ __launch_bounds__(KR_SCAN_NT) void k_key_record_scan(const u32* __restrict__ kdist, u32 tiles,
                                                                u32* __restrict__ roff, u64* __restrict__ host_total,
                                                                u32 seq) {
    __shared__ u32 scan[KR_SCAN_NT];
    const int tid = threadIdx.x;
    const u32 per = (tiles + KR_SCAN_NT - 1) / KR_SCAN_NT;
    const u32 lo = min((u32)tid * per, tiles), hi = min(lo + per, tiles);
    u32 mine = 0;
    for (u32 s = lo; s < hi; ++s) mine += kdist[s];
    scan[tid] = mine;
    __syncthreads();
    for (int o = 1; o < KR_SCAN_NT; o <<= 1) {   // inclusive scan
        const u32 v = tid >= o ? scan[tid - o] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    u32 run = scan[tid] - mine;
    for (u32 s = lo; s < hi; ++s) {
        roff[s] = run;
        run += kdist[s];
    }
    if (tid == KR_SCAN_NT - 1) {
        roff[tiles] = scan[tid];
        __hip_atomic_store(host_total, ((u64)seq << 32) | scan[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The records of one cached slot (a workgroup each, once per generation): the
// first pixel of each winner in p order builds the winner's record, with the
// helpers k_keys_idx builds it with, at its dense number in the slot's part of
// the store.
__global__ __launch_bounds__(KI_NT) void k_key_records(const FrameParams fp, const u64* __restrict__ kkeys, u32 tiles,
                                                       const unsigned short* __restrict__ kidx,
                                                       const u32* __restrict__ roff, f64* __restrict__ krec) {
    constexpr int MODE = ATTR_GOURAUD;
    constexpr int REC = RecLen<MODE>::REC;
    __shared__ u32 first[TH * TW];   // per dense number: the winner's first pixel
    const u32 slot = blockIdx.x;
    if (slot >= tiles) return;
    const int tid = threadIdx.x;
    for (int i = tid; i < TH * TW; i += KI_NT) first[i] = ~0u;
    __syncthreads();
    const unsigned short* const six = kidx + (size_t)slot * (TH * TW);
    const u64* const src = kkeys + (size_t)slot * (TH * TW);
    const u32 base = roff[slot], count = roff[slot + 1] - base;
    unsigned short d[KI_PPT];
#pragma unroll
    for (int k = 0; k < KI_PPT; ++k) {
        const int p = tid + k * KI_NT;
        d[k] = six[p];
        if (d[k] < count) atomicMin(&first[d[k]], (u32)p);   // (KI_NONE is past every count)
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < KI_PPT; ++k) {
        const int p = tid + k * KI_NT;
        if (d[k] >= count || first[d[k]] != (u32)p) continue;
        const u32 id = (u32)src[p];
        f64 r[REC];
        make_record<MODE>(fp, (i64)id - 1, r);
        f64* const dst = krec + ((size_t)base + d[k]) * REC;
#pragma unroll
        for (int j = 0; j < REC; ++j) dst[j] = r[j];
    }
}

// What a k_keys_idx instance writes (its head comment below).
enum { KO_ALL = 0, KO_FRAME = 1, KO_RESOLVE = 2 };

// A shaded pixel's value, by OUT: framebuffer + frame output, the frame output alone, or the framebuffer alone.
template <int OUT>
__device__ __forceinline__ void keys_idx_out(const FrameParams& fp, i64 p, i64 px, i64 py, f64 cr, f64 cg, f64 cb,
                                             f64 ca) {
    if constexpr (OUT == KO_ALL) {
        store_colour(fp, p, px, py, cr, cg, cb, ca);
    } else if constexpr (OUT == KO_FRAME) {
        store_frame_out(fp, p, px, py, cr, cg, cb, ca);
    } else {   // (store_colour's f64 stores)
        const int ipp = fp.ipp;
        f64* dst = fp.fb + p * ipp;
        out_store<f64>(dst, cr); out_store<f64>(dst + 1, cg); out_store<f64>(dst + 2, cb);
        if (ipp == 4) out_store<f64>(dst + 3, ca);
    }
}

// The steady kernel of a cached Gouraud batch whose generation has its index
// (launch_vis): k_keys' items, grid and empty-tile path; a cached item as the
// head comment above says.  Every value is formed by nr_tri_shade.h's helpers
// as shade_tile forms it, so a frame is the one k_keys gives, bit for bit.
// LDS: the KI_RT records alone (35 KB: four 256-thread workgroups per CU).
//
// OUT: what a cached item writes (deferred stores).
//   KO_ALL      everything, as above: the kernel as it was before the parameter (its code is unchanged).
//   KO_FRAME    the frame output alone -- no key loads in the first round, no depth and no f64 stores: the
//               steady kernel of a batch whose framebuffer and depth values stay pending (DeferredStores).  Only
//               a KI_DIRECT pixel reads its key, for the id.
//   KO_RESOLVE  the pending values of such a batch, when something needs the buffers, from the batch's own
//               snapshot: the f64 values where fp.fb is set, the depths where fp.depth is (launch_keys_resolve
//               clears the pointer of a half that is not wanted); no frame output, no tile stamp, empty items
//               skipped (k_tile_clear owns those tiles).  A depth-only resolve builds no records.
// A deferred batch has a uniform colour clear pending (fp.frameU8 is set only then), so apply_winner's read of
// the destination (ca != 1 and no clear pending) is never reached on a deferred batch or its resolve: the f64
// values a KO_FRAME launch leaves unwritten are read by neither.  KO_FRAME then KO_RESOLVE form every value by
// the same helpers in the same order as KO_ALL: the buffers end up the same bit for bit.
constexpr int KI_OVF_Q = 1;   // directly loaded records in flight per thread (their ids come from the keys again)
template <int ZMODE, int MODEW, int NT, int OUT = KO_ALL>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(VIS_WPE))) void k_keys_idx(
    const FrameParams fp, const uint4* __restrict__ items, const u64* __restrict__ kkeys, const u32* __restrict__ kplan,
    const unsigned short* __restrict__ kidx, const u32* __restrict__ kwin, const u32* __restrict__ kcnt) {
    constexpr int MODE = attr_base(MODEW);
    static_assert(MODE == ATTR_GOURAUD && !attr_wraps(MODEW), "Gouraud batches only");
    constexpr int REC = RecLen<MODE>::REC;
    constexpr int PPT = TH * TW / NT;
    static_assert(PPT <= 32, "overflow bitmask");
    __shared__ __attribute__((aligned(16))) f64 rec[KI_RT * REC];
    if constexpr (OUT != KO_RESOLVE) raster_stamp_begin(fp);
    const u32 nitems = kplan[1];
    uint4 dnext = blockIdx.x < nitems ? items[blockIdx.x] : make_uint4(0, 0, 0, 0);
#if NR_PROBE
    const int tid = threadIdx.x;
    u64 pr_t0 = 0;
    u32 pr_item = ~0u;
    uint4 pr_d = make_uint4(0, 0, 0, 0);
#endif
    for (u32 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const uint4 d = dnext;
        if (item + gridDim.x < nitems) dnext = items[item + gridDim.x];
#if NR_PROBE
        if (tid == 0) {   // (the record's list range: [0, kept pairs))
            const u64 now = __builtin_amdgcn_s_memrealtime();
            if (pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, now, NT);
            pr_t0 = now; pr_item = item; pr_d = make_uint4(d.x, 0u, d.z, 1u);
        }
#endif
        __syncthreads();   // (the last item's pixels have read its records)
        const int itid = opaque_tid();
        const int tile = (int)d.x;
        const int tx = tile % fp.tiles_x, ty = tile / fp.tiles_x;
        const i64 x0 = (i64)tx * TW, y0 = (i64)ty * TH;
        const int wlim = (int)(fp.W - x0 < TW ? fp.W - x0 : TW);
        const int hlim = (int)(fp.H - y0 < TH ? fp.H - y0 : TH);
        if (d.y == ~0u) {   // no kept pair: only the pending clears (as k_vis)
            if constexpr (OUT == KO_RESOLVE) continue;
            if (fp.tileStamp) {
                if (fp.frameU8 && fp.pendColor) {
                    const f64 v = fp.pendColorValue;
                    for (int p = itid; p < TH * TW; p += NT) {
                        const int lx = p & (TW - 1), ly = p / TW;
                        if (lx < wlim && ly < hlim)
                            store_frame_out(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly, v, v, v, v);
                    }
                }
                if (itid == 0) fp.tileStamp[tile] = fp.tileEpoch;
                continue;
            }
            for (int p = itid; p < TH * TW; p += NT) {
                const int lx = p & (TW - 1), ly = p / TW;
                if (lx < wlim && ly < hlim)
                    store_clear<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly);
            }
            continue;
        }
        // every load of the item's first round in flight together: the keys, the
        // two winners whose records this thread builds, the index entries
        const size_t slot = (u32)__builtin_amdgcn_readfirstlane((int)d.y);   // (uniform: the count is a scalar load)
        const u64* const src = kkeys + slot * (TH * TW);
        const unsigned short* const six = kidx + slot * (TH * TW);
        const u32* const swin = kwin + slot * KI_RT;
        u64 kv[PPT];
        unsigned short di[PPT];
        if constexpr (OUT == KO_RESOLVE) {
            if (!fp.fb) {   // depths alone: from the keys, no records
#pragma unroll
                for (int k = 0; k < PPT; ++k) kv[k] = src[itid + k * NT];
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const int p = itid + k * NT, lx = p & (TW - 1), ly = p / TW;
                    if (lx >= wlim || ly >= hlim) continue;
                    store_depth<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, kv[k]);
                }
                continue;
            }
        }
        if constexpr (OUT != KO_FRAME) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) kv[k] = src[itid + k * NT];
        }
        // (unconditional loads from in-range addresses, as k_vis' chunk loads: a conditional load makes the
        // compiler wait for everything in flight on the spot.  Entries past the slot's count are never used)
        const u32 w0 = swin[itid < KI_RT ? itid : 0];
        const u32 w1 = swin[itid + NT < KI_RT ? itid + NT : 0];
        const u32 U = min(kcnt[2 * slot], (u32)KI_RT);
#pragma unroll
        for (int k = 0; k < PPT; ++k) di[k] = six[itid + k * NT];
        NR_PROBE_STAMP(1);
        NR_PROBE_STAMP(2);
        if constexpr (OUT == KO_ALL) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int p = itid + k * NT, lx = p & (TW - 1), ly = p / TW;
                if (lx >= wlim || ly >= hlim) continue;
                store_depth<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, kv[k]);
            }
        } else if constexpr (OUT == KO_RESOLVE) {
            if (fp.depth) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const int p = itid + k * NT, lx = p & (TW - 1), ly = p / TW;
                    if (lx >= wlim || ly >= hlim) continue;
                    store_depth<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, kv[k]);
                }
            }
        }
        NR_PROBE_STAMP(4);
        static_assert(KI_RT <= 2 * NT, "two winners per thread cover the staged records");
        {   // one record per staged winner, every thread's loads issued (a thread past the count reads triangle
            // 0's data and builds nothing); the few winners past NT (a 256-thread workgroup's last 24) in a
            // second round
            const u32 u = (u32)itid;
            RecordSrc<MODE> s0;
            load_record_src<MODE>(fp, u < U ? (i64)w0 - 1 : 0, s0);
            if (u < U) build_record<MODE>(fp, s0, rec + u * REC);
            if (U > (u32)NT && u + NT < U) {
                RecordSrc<MODE> s1;
                load_record_src<MODE>(fp, (i64)w1 - 1, s1);
                build_record<MODE>(fp, s1, rec + (u + NT) * REC);
            }
        }
        __syncthreads();
        NR_PROBE_STAMP(5);
        const TexView& tv = fp.tex;
        u32 ovf = 0;   // bit k: pixel k's winner is not staged
#pragma unroll 1
        for (int k = 0; k < PPT; ++k) {
            const int p = itid + k * NT, lx = p & (TW - 1), ly = p / TW;
            if (lx >= wlim || ly >= hlim) continue;
            const i64 px = x0 + lx, py = y0 + ly;
            const i64 gp = py * fp.W + px;
            u32 dn = KI_NONE;
#pragma unroll
            for (int q = 0; q < PPT; ++q)
                if (q == k) dn = di[q];   // static register index
            if (dn == KI_NONE) {
                if (fp.pendColor) {
                    const f64 v = fp.pendColorValue;
                    keys_idx_out<OUT>(fp, gp, px, py, v, v, v, v);
                }
                continue;
            }
            if (dn >= U) {   // KI_DIRECT
                ovf |= 1u << k;
                continue;
            }
            f64 cr, cg, cb, ca;
            record_colour<MODE>(tv, rec + dn * REC, px, py, cr, cg, cb, ca);
            apply_winner(fp, gp, cr, cg, cb, ca);
            keys_idx_out<OUT>(fp, gp, px, py, cr, cg, cb, ca);
        }
        NR_PROBE_STAMP(6);   // (probe builds: the pixel pass ends, the overflow loop begins)
        // pixels whose winner is not staged (shade_tile's pass 3b), KI_OVF_Q at
        // a time: their ids' loads in flight together, then their records'
#pragma unroll 1
        while (ovf) {
            int kq[KI_OVF_Q];
            u32 wid[KI_OVF_Q];
            RecordSrc<MODE> rs[KI_OVF_Q];
#pragma unroll
            for (int j = 0; j < KI_OVF_Q; ++j) {
                kq[j] = -1;
                wid[j] = 0;
                if (!ovf) continue;
                kq[j] = __builtin_ctz(ovf);
                ovf &= ovf - 1;
                wid[j] = (u32)src[itid + kq[j] * NT];   // (the key again: eight ids kept live measured no faster)
            }
#pragma unroll
            for (int j = 0; j < KI_OVF_Q; ++j)
                if (kq[j] >= 0) load_record_src<MODE>(fp, (i64)wid[j] - 1, rs[j]);
#pragma unroll
            for (int j = 0; j < KI_OVF_Q; ++j) {
                if (kq[j] < 0) continue;
                const int p = itid + kq[j] * NT, lx = p & (TW - 1), ly = p / TW;
                const i64 px = x0 + lx, py = y0 + ly;
                const i64 gp = py * fp.W + px;
                f64 r[REC];
                build_record<MODE>(fp, rs[j], r);
                f64 cr, cg, cb, ca;
                record_colour<MODE>(tv, r, px, py, cr, cg, cb, ca);
                apply_winner(fp, gp, cr, cg, cb, ca);
                keys_idx_out<OUT>(fp, gp, px, py, cr, cg, cb, ca);
            }
        }
    }
#if NR_PROBE
    if (tid == 0 && pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, __builtin_amdgcn_s_memrealtime(), NT);
#endif
    if constexpr (OUT != KO_RESOLVE) raster_stamp_end(fp);
}

// The steady kernel of a cached Gouraud batch whose generation has its records
// (launch_vis): k_keys_idx' items, grid, empty-item path, pixel pass and
// outputs (OUT: KO_ALL or KO_FRAME; a resolve stays with k_keys_idx), but a
// cached item's records come from the generation's record store (KeyRecords),
// where k_key_records left them built by the same helpers: the staged ones as
// one coalesced copy into LDS -- its addresses depend on the item's two record
// offsets alone, so the winner ids, the gather of their sources and the build
// are gone from the item's dependent chain, which is {item, offsets} -> records
// (work units, below) -- and the record of a pixel whose
// dense number is KR_RT or more straight from the store, by that number: no
// key, no gather, no build.
//
// Work units (nr_free.h keys_rec_units; the grid is their count, and the kernel
// strides over them whatever the grid): unit v < nc is cached item v, whose slot
// is v (k_key_plan), so the record offsets are loaded beside the item and not
// behind it; a unit from nc on is a run of NT / 64 empty items, one per wave
// (keys_rec_empty).  nc, nit: the key plan's totals {cached tiles, items} as the
// host has seen them (kplan's words, by value: no load of them ahead of the item's).
//
// LDS: KR_RT records at a stride of KR_LU 16-byte units (35 712 B: four
// 256-thread workgroups per CU).
constexpr int KR_OVF_Q = 2;   // directly loaded records in flight per thread

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

// The pending clear of an empty item (no kept pair: as k_keys_idx' empty-tile path), by one wave: lane 0..63.
// Under a tile stamp only the frame output is written, and every byte of it is one of three constants (the
// pending colour is uniform: Y, U, V; under RGB one byte value).  A tile wholly inside the frame whose rows'
// byte addresses in the frame output are 16-byte aligned is written in 16-byte words; every other tile pixel
// by pixel, with store_frame_out.
template <int ZMODE>
__device__ __forceinline__ void keys_rec_empty(const FrameParams& fp, int tile, int lane) {
    const int tx = tile % fp.tiles_x, ty = tile / fp.tiles_x;
    const i64 x0 = (i64)tx * TW, y0 = (i64)ty * TH;
    const int wlim = (int)(fp.W - x0 < TW ? fp.W - x0 : TW);
    const int hlim = (int)(fp.H - y0 < TH ? fp.H - y0 : TH);
    if (!fp.tileStamp) {
        for (int p = lane; p < TH * TW; p += 64) {
            const int lx = p & (TW - 1), ly = p / TW;
            if (lx < wlim && ly < hlim) store_clear<ZMODE>(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly);
        }
        return;
    }
    if (fp.frameU8 && fp.pendColor) {
        const f64 v = fp.pendColorValue;
        const bool inside = wlim == TW && hlim == TH && !(reinterpret_cast<uintptr_t>(fp.frameU8) & 15);
        const int b8 = nr_to_u8(v);
        if (inside && fp.frameYUV && !(fp.W & 31)) {
            // Y: TH rows of TW / 16 words; U, V: TH / 2 rows of TW / 32 words each (W is a multiple of 32, so
            // the planes' bases W * H and W * H + (W / 2) * (H / 2) and the chroma rows are aligned as well)
            constexpr int YW = TH * TW / 16, CW = TH * TW / 64;
            static_assert(YW % 64 == 0 && 2 * CW == 64, "two words of Y and one of chroma per lane");
            const u32 yb = nr_y_of(b8, b8, b8) * 0x01010101u, ub = nr_u_of(b8, b8, b8) * 0x01010101u;
            const u32 vb = nr_v_of(b8, b8, b8) * 0x01010101u;
#pragma unroll
            for (int j = 0; j < YW / 64; ++j) {
                const int w = lane + 64 * j;
                iu8* const q = fp.frameU8 + (y0 + w / (TW / 16)) * fp.W + x0 + (w % (TW / 16)) * 16;
                out_store<u32x4>(reinterpret_cast<u32x4*>(q), u32x4{yb, yb, yb, yb});
            }
            const i64 cw = fp.W >> 1;
            const int w = lane & (CW - 1);
            iu8* q = fp.frameU8 + fp.W * fp.H + ((y0 >> 1) + w / (TW / 32)) * cw + (x0 >> 1) + (w % (TW / 32)) * 16;
            if (lane >= CW) q += cw * (fp.H >> 1);
            const u32 cb = lane >= CW ? vb : ub;
            out_store<u32x4>(reinterpret_cast<u32x4*>(q), u32x4{cb, cb, cb, cb});
        } else if (inside && !fp.frameYUV && !((fp.W * fp.ipp) & 15)) {
            // TH rows of TW * ipp / 16 words (12 or 16): six or eight words per lane
            const int wpr = TW * fp.ipp / 16, words = TH * wpr;
            const u32 cb = (u32)b8 * 0x01010101u;
#pragma unroll
            for (int j = 0; j < TH * TW * 4 / 16 / 64; ++j) {
                const int w = lane + 64 * j;
                iu8* const q = fp.frameU8 + ((y0 + w / wpr) * fp.W + x0) * fp.ipp + (w % wpr) * 16;
                if (w < words) out_store<u32x4>(reinterpret_cast<u32x4*>(q), u32x4{cb, cb, cb, cb});
            }
        } else {
            for (int p = lane; p < TH * TW; p += 64) {
                const int lx = p & (TW - 1), ly = p / TW;
                if (lx < wlim && ly < hlim)
                    store_frame_out(fp, (y0 + ly) * fp.W + x0 + lx, x0 + lx, y0 + ly, v, v, v, v);
            }
        }
    }
    if (lane == 0) fp.tileStamp[tile] = fp.tileEpoch;
}

template <int ZMODE, int MODEW, int NT, int OUT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(VIS_WPE))) void k_keys_rec(
    const FrameParams fp, const uint4* __restrict__ items, const u64* __restrict__ kkeys, const u32 nc, const u32 nit,
    const unsigned short* __restrict__ kidx, const u32* __restrict__ roff, const f64* __restrict__ krec) {
    constexpr int MODE = attr_base(MODEW);
    static_assert(MODE == ATTR_GOURAUD && !attr_wraps(MODEW), "Gouraud batches only");
    static_assert(OUT == KO_ALL || OUT == KO_FRAME, "a resolve runs k_keys_idx");
    constexpr int REC = RecLen<MODE>::REC;
    static_assert(REC % 2 == 0, "records are copied in 16-byte units");
    constexpr int RU = REC / 2;                  // 16-byte units of a record
    constexpr int LU = KR_LU;                    // ... of its place in LDS
    static_assert(LU >= RU && (RU & (RU - 1)) == 0, "a padded record; the unit's place by shifts");
    constexpr int UNITS = KR_RT * RU;            // ... of the staged records
    constexpr int CPT = (UNITS + NT - 1) / NT;   // ... of a thread's share of them
    constexpr int PPT = TH * TW / NT;
    constexpr int RSTEP = NT / TW;               // rows between a thread's pixels: p = itid + k * NT is one column
    static_assert(PPT <= 32, "overflow bitmask");
    static_assert(NT % TW == 0 && PPT % 2 == 0, "a column per thread; index entries in pairs");
    constexpr int EW = NT / 64;                  // empty items of a unit
    __shared__ __attribute__((aligned(16))) double2 rec[KR_RT * LU];
    raster_stamp_begin(fp);
    const u32 units = nc + (nit - nc + EW - 1) / EW;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    auto item_of = [&](u32 v) { return v < nc ? v : nc + (v - nc) * EW + wave; };   // (past nit: nothing to do)
    uint4 dnext = make_uint4(0, 0, 0, 0);
    if (blockIdx.x < units && item_of(blockIdx.x) < nit) dnext = items[item_of(blockIdx.x)];
#if NR_PROBE
    const int tid = threadIdx.x;
    u64 pr_t0 = 0;
    u32 pr_item = ~0u;
    uint4 pr_d = make_uint4(0, 0, 0, 0);
#endif
    for (u32 v = blockIdx.x; v < units; v += gridDim.x) {
        const uint4 d = dnext;
        const u32 item = item_of(v);
        if (v + gridDim.x < units && item_of(v + gridDim.x) < nit) dnext = items[item_of(v + gridDim.x)];
#if NR_PROBE
        if (tid == 0) {
            const u64 now = __builtin_amdgcn_s_memrealtime();
            if (pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, now, NT);
            pr_t0 = now; pr_item = item; pr_d = make_uint4(d.x, 0u, d.z, 1u);
        }
#endif
        const int itid = opaque_tid();
        if (v >= nc) {   // a run of empty items: only the pending clears, a wave each
            if (item < nit) keys_rec_empty<ZMODE>(fp, (int)d.x, itid & 63);
            continue;
        }
        __syncthreads();   // (the last item's pixels have read its records)
        // every load of the item in flight together: the index entries, (KO_ALL) the keys, and this thread's
        // share of the slot's staged records.  Unconditional loads from in-range addresses (as k_keys_idx): a
        // unit past the slot's staged records reads their last unit again -- the same line, no new bytes -- or,
        // in a slot without winners, the store's tail (nr_key_records.h room_doubles)
        const size_t slot = v;   // (uniform: the offsets are scalar loads, in flight beside the item's)
        const u64* const src = kkeys + slot * (TH * TW);
        const unsigned short* const six = kidx + slot * (TH * TW);
        const u32 r0 = roff[slot], r1 = roff[slot + 1];
        const u32 U = min(r1 - r0, (u32)KR_RT);
        const f64* const sbase = krec + (size_t)r0 * REC;
        const double2* const srec = reinterpret_cast<const double2*>(sbase);
        const u32 ulast = max(U * RU, 1u) - 1;
        u64 kv[PPT];
        unsigned short di[PPT];
        double2 cp[CPT];
        if constexpr (OUT == KO_ALL) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) kv[k] = src[itid + k * NT];
        }
#pragma unroll
        for (int j = 0; j < CPT; ++j) cp[j] = srec[min((u32)(itid + j * NT), ulast)];
#pragma unroll
        for (int k = 0; k < PPT; ++k) di[k] = six[itid + k * NT];
        NR_PROBE_STAMP(1);
        NR_PROBE_STAMP(2);
        const int tile = (int)d.x;
        const int tx = tile % fp.tiles_x, ty = tile / fp.tiles_x;
        const int lx = itid & (TW - 1), ly0 = itid / TW;
        const int xi = tx * TW + lx, yi0 = ty * TH + ly0;   // the thread's column and its first row (below 2^31)
        const int wlim = (int)(fp.W - (i64)tx * TW < TW ? fp.W - (i64)tx * TW : TW);
        const int hlim = (int)(fp.H - (i64)ty * TH < TH ? fp.H - (i64)ty * TH : TH);
        const i64 gp0 = (i64)yi0 * fp.W + xi, gstep = (i64)RSTEP * fp.W;
        if constexpr (OUT == KO_ALL) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                if (lx >= wlim || ly0 + k * RSTEP >= hlim) continue;
                store_depth<ZMODE>(fp, gp0 + k * gstep, kv[k]);
            }
        }
        NR_PROBE_STAMP(4);
        // the loaded units pinned here, all of them: without it the compiler sinks each load into the block of
        // its guarded store below and waits for it there -- CPT dependent memory rounds in place of one
#pragma unroll
        for (int j = 0; j < CPT; ++j) asm volatile("" : "+v"(cp[j].x), "+v"(cp[j].y));
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const u32 u = (u32)(itid + j * NT);
            if (u < U * RU) rec[(u / RU) * LU + (u & (RU - 1))] = cp[j];
        }
        // the index entries in pairs, as a ring of PPT / 2 words that the pixel loop turns by one entry per
        // pixel: no select chain over the eight registers, and after PPT turns the ring is as it was
        u32 dw[PPT / 2];
#pragma unroll
        for (int q = 0; q < PPT / 2; ++q) dw[q] = (u32)di[2 * q] | ((u32)di[2 * q + 1] << 16);
        __syncthreads();
        NR_PROBE_STAMP(5);
        const TexView& tv = fp.tex;
        u32 ovf = 0;   // bit k: pixel k's winner is not staged
        i64 gp = gp0 - gstep;
#pragma unroll 1
        for (int k = 0; k < PPT; ++k) {
            gp += gstep;
            const u32 dn = dw[0] & 0xFFFFu;
            {
                const u32 first = dw[0];
#pragma unroll
                for (int q = 0; q + 1 < PPT / 2; ++q) dw[q] = __builtin_amdgcn_alignbit(dw[q + 1], dw[q], 16);
                dw[PPT / 2 - 1] = __builtin_amdgcn_alignbit(first, dw[PPT / 2 - 1], 16);
            }
            const int yi = yi0 + k * RSTEP;
            if (lx >= wlim || ly0 + k * RSTEP >= hlim) continue;
            const i64 px = xi, py = yi;
            if (dn == KI_NONE) {
                if (fp.pendColor) {
                    const f64 v = fp.pendColorValue;
                    keys_idx_out<OUT>(fp, gp, px, py, v, v, v, v);
                }
                continue;
            }
            if (dn >= U) {
                ovf |= 1u << k;
                continue;
            }
            // the record's eight reads issued before the first use (pinned: left alone, the compiler reads it
            // in four groups through the same registers, with a wait behind each)
            double2 rr[RU];
#pragma unroll
            for (int i = 0; i < RU; ++i) rr[i] = rec[dn * LU + i];
#pragma unroll
            for (int i = 0; i < RU; ++i) asm volatile("" : "+v"(rr[i].x), "+v"(rr[i].y));
            f64 r[REC];
#pragma unroll
            for (int i = 0; i < RU; ++i) { r[2 * i] = rr[i].x; r[2 * i + 1] = rr[i].y; }
            f64 cr, cg, cb, ca;
            record_colour<MODE>(tv, r, px, py, cr, cg, cb, ca);
            apply_winner(fp, gp, cr, cg, cb, ca);
            keys_idx_out<OUT>(fp, gp, px, py, cr, cg, cb, ca);
        }
        NR_PROBE_STAMP(6);
        // pixels whose winner is not staged, KR_OVF_Q at a time: their records' loads in flight together (a
        // thread with fewer left reads the slot's first record again and shades nothing from it)
#pragma unroll 1
        while (ovf) {
            int kq[KR_OVF_Q];
            double2 r2[KR_OVF_Q][RU];
#pragma unroll
            for (int j = 0; j < KR_OVF_Q; ++j) {
                kq[j] = -1;
                u32 dn = 0;
                if (ovf) {
                    kq[j] = __builtin_ctz(ovf);
                    ovf &= ovf - 1;
                    u32 w = 0;
#pragma unroll
                    for (int q = 0; q < PPT / 2; ++q)
                        if (q == kq[j] >> 1) w = dw[q];   // static register index (the ring is back at its start)
                    dn = (w >> ((kq[j] & 1) * 16)) & 0xFFFFu;
                }
                const double2* const q2 = srec + (size_t)dn * RU;
#pragma unroll
                for (int i = 0; i < RU; ++i) r2[j][i] = q2[i];
            }
#pragma unroll
            for (int j = 0; j < KR_OVF_Q; ++j) {
                if (kq[j] < 0) continue;
                const i64 px = xi, py = yi0 + kq[j] * RSTEP;
                const i64 gp = gp0 + kq[j] * gstep;
                f64 r[REC];
#pragma unroll
                for (int i = 0; i < RU; ++i) { r[2 * i] = r2[j][i].x; r[2 * i + 1] = r2[j][i].y; }
                f64 cr, cg, cb, ca;
                record_colour<MODE>(tv, r, px, py, cr, cg, cb, ca);
                apply_winner(fp, gp, cr, cg, cb, ca);
                keys_idx_out<OUT>(fp, gp, px, py, cr, cg, cb, ca);
            }
        }
    }
#if NR_PROBE
    if (tid == 0 && pr_item != ~0u) probe_item(pr_item, pr_d, pr_t0, __builtin_amdgcn_s_memrealtime(), NT);
#endif
    raster_stamp_end(fp);
}

// The instance of a batch among its four shapes -- wide workgroups (never a counting batch) or not, the flattened
// raster or not -- MARK: a marking frame's.
template <int Z, bool C, int G, bool MARK>
auto vis_kernel(bool wide, bool coop) {
    if (wide) return coop ? k_vis<Z, false, G, true, 2 * VWG, MARK> : k_vis<Z, false, G, false, 2 * VWG, MARK>;
    return coop ? k_vis<Z, C, G, true, VWG, MARK> : k_vis<Z, C, G, false, VWG, MARK>;
}

// NR_KEYS_WIDE=1 (tests, A/B): every batch shaded from the key cache runs k_keys' 512-thread instance.
static bool keys_wide_forced() {
    static const bool v = [] {
        const char* e = getenv("NR_KEYS_WIDE");
        return e && atoi(e) == 1;
    }();
    return v;
}

// t: the totals that pick the variant -- this batch's when they are known (a
// warm, known-size or exact batch), else the last validated batch's
template <int Z, bool C, int G>
void launch_vis(const FrameParams& fp, const TriScratch& sc, const BatchTotals& t, const VisArgs& va, u32 grid,
                hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    // the flattened raster when the batch has more than COOP_PAIRS tiles per
    // triangle (large triangles), or when there is no history
    const bool coop = sc.coopMode ? sc.coopMode == 1 : (t.n == 0 || (u64)t.pairs > (u64)(COOP_PAIRS * (f64)t.n));
    // wide workgroups when the batch has few pairs (a sharded frame): its
    // dense items run at low occupancy and are latency-bound
    const bool wide = !C && t.n != 0 && t.heavy > 0 && t.heavy < WIDE_HEAVY;
    auto kernel = vis_kernel<Z, C, G, false>(wide, coop);
    // a marking frame (fp.winMask; never a counting batch, never LESS without write -- and only a repeat
    // TriangleBuffer draw marks, which has no q: the filtered perspective mode and the modulated modes have no
    // marking instance)
    // The key cache's batches are those of a pruned list, so they too exist only where a marking frame does.  A
    // cached batch runs k_keys at the workgroup size k_vis would take; the capture frame (one per generation) the
    // narrow capturing instance of its raster shape.
    bool narrow = false;
    if constexpr (!C && Z != 2 && attr_base(G) != ATTR_TEX_PERSP_BIL && !attr_modulated(attr_base(G))) {
        if (va.kkeys) {
            const bool w = wide || keys_wide_forced();
            if constexpr (G == ATTR_GOURAUD) {
                if (va.kindex.idx && va.krec.rec) {   // (... and its records, and SetKeyRecords is on)
                    // a workgroup per work unit: the cached items, then the empty ones in runs (keys_rec_units)
                    const u32 nc = va.krec.cached, nit = va.krec.items;
                    const u32 rgrid = std::min<u32>(std::max<u32>(keys_rec_units(nc, nit, w), 1), 8192);
                    if (va.defer)
                        hipExtLaunchKernelGGL(w ? k_keys_rec<Z, G, 2 * VWG, KO_FRAME> : k_keys_rec<Z, G, VWG, KO_FRAME>,
                                              dim3(rgrid), dim3(w ? 2 * VWG : VWG), 0, s, start, stop, 0, fp, va.kitems,
                                              va.kkeys, nc, nit, va.kindex.idx, va.krec.roff, va.krec.rec);
                    else
                        hipExtLaunchKernelGGL(w ? k_keys_rec<Z, G, 2 * VWG, KO_ALL> : k_keys_rec<Z, G, VWG, KO_ALL>,
                                              dim3(rgrid), dim3(w ? 2 * VWG : VWG), 0, s, start, stop, 0, fp, va.kitems,
                                              va.kkeys, nc, nit, va.kindex.idx, va.krec.roff, va.krec.rec);
                    return;
                }
                if (va.kindex.idx) {   // (the generation has its index, and SetKeyIndex is on: pruned_enqueue)
                    if (va.defer) {   // (its f64 and depth stores stay pending: DeferredStores)
                        hipExtLaunchKernelGGL(w ? k_keys_idx<Z, G, 2 * VWG, KO_FRAME> : k_keys_idx<Z, G, VWG, KO_FRAME>,
                                              dim3(grid), dim3(w ? 2 * VWG : VWG), 0, s, start, stop, 0, fp, va.kitems,
                                              va.kkeys, va.kplan, va.kindex.idx, va.kindex.win, va.kindex.cnt);
                        return;
                    }
                    hipExtLaunchKernelGGL(w ? k_keys_idx<Z, G, 2 * VWG> : k_keys_idx<Z, G, VWG>, dim3(grid),
                                          dim3(w ? 2 * VWG : VWG), 0, s, start, stop, 0, fp, va.kitems, va.kkeys, va.kplan,
                                          va.kindex.idx, va.kindex.win, va.kindex.cnt);
                    return;
                }
            }
            hipExtLaunchKernelGGL(w ? k_keys<Z, G, 2 * VWG> : k_keys<Z, G, VWG>, dim3(grid), dim3(w ? 2 * VWG : VWG), 0, s,
                                  start, stop, 0, fp, va.kitems, va.kkeys, va.kplan);
            return;
        }
        if (va.capture) {   // (fp.kcap shares fp.winMask's place: asked first)
            kernel = coop ? k_vis<Z, false, G, true, VWG, false, true> : k_vis<Z, false, G, false, VWG, false, true>;
            narrow = true;
        } else if (fp.winMask) {
            kernel = vis_kernel<Z, false, G, true>(wide, coop);
        }
    }
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(wide && !narrow ? 2 * VWG : VWG), 0, s, start, stop, 0, fp, va.items,
                          va.list, sc.kslot.p, sc.fdone.p, va.plan, WarmCheck{va.wc});
}

}  // namespace

// k_vis' ZMODE of a batch: 0 no test, 1 LESS + write, 2 LESS without write
int z_mode(const FrameParams& fp) { return fp.depthTest ? (fp.depthWrite ? 1 : 2) : 0; }

void launch_key_index(const uint4* kitems, const u64* kkeys, u32 tiles, unsigned short* idx, u32* win, u32* cnt,
                      u32* dist, i64 W, i64 H, int tiles_x, hipStream_t s) {
    if (!tiles) return;
    hipLaunchKernelGGL(k_key_index, dim3(tiles), dim3(KI_NT), 0, s, kitems, kkeys, tiles, idx, win, cnt, dist, W, H,
                       tiles_x);
}

void launch_key_record_scan(const u32* dist, u32 tiles, u32* roff, u64* host_total, u32 seq, hipStream_t s) {
    hipLaunchKernelGGL(k_key_record_scan, dim3(1), dim3(KR_SCAN_NT), 0, s, dist, tiles, roff, host_total, seq);
}

void launch_key_records(const FrameParams& fp, const u64* kkeys, u32 tiles, const unsigned short* idx, const u32* roff,
                        f64* rec, hipStream_t s) {
    if (!tiles) return;
    hipLaunchKernelGGL(k_key_records, dim3(tiles), dim3(KI_NT), 0, s, fp, kkeys, tiles, idx, roff, rec);
}

bool keys_wide(const BatchTotals& t) {   // (launch_vis' choice for a batch shaded from the key cache)
    return (t.n != 0 && t.heavy > 0 && t.heavy < WIDE_HEAVY) || keys_wide_forced();
}

void launch_keys_resolve(const FrameParams& fp, const VisArgs& va, u32 grid, bool wide, bool colour, bool depth,
                         hipStream_t s) {
    const int zmode = z_mode(fp);
    FrameParams fr = fp;   // (the kernel writes the halves whose destination it is given)
    if (!colour) fr.fb = nullptr;
    if (!depth || zmode != 1) fr.depth = nullptr;
    if ((!fr.fb && !fr.depth) || !grid || zmode == 2) return;
    auto kernel = wide ? k_keys_idx<0, ATTR_GOURAUD, 2 * VWG, KO_RESOLVE> : k_keys_idx<0, ATTR_GOURAUD, VWG, KO_RESOLVE>;
    if (zmode == 1)
        kernel = wide ? k_keys_idx<1, ATTR_GOURAUD, 2 * VWG, KO_RESOLVE> : k_keys_idx<1, ATTR_GOURAUD, VWG, KO_RESOLVE>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(wide ? 2 * VWG : VWG), 0, s, fr, va.kitems, va.kkeys, va.kplan,
                       va.kindex.idx, va.kindex.win, va.kindex.cnt);
}

void launch_vis_any(const FrameParams& fp, const TriScratch& sc, const BatchTotals& t, const VisArgs& va,
                    u32 grid, hipStream_t s, hipEvent_t start, hipEvent_t stop) {
    // (a textured batch with a wrapped axis takes its mode's ATTR_WRAPS instance)
    const int zmode = z_mode(fp), mode = fp.src.mode | (attr_textured(fp.src.mode) && fp.wrap().any() ? ATTR_WRAPS : 0);
#define NR_VG(ZM, G) (fp.fragCounter ? launch_vis<ZM, true, G>(fp, sc, t, va, grid, s, start, stop) \
                                     : launch_vis<ZM, false, G>(fp, sc, t, va, grid, s, start, stop))
#define NR_VZ(ZM)                                            \
    (mode == (ATTR_TEXC_BIL | ATTR_WRAPS) ? NR_VG(ZM, ATTR_TEXC_BIL | ATTR_WRAPS)        \
     : mode == (ATTR_TEXC | ATTR_WRAPS)    ? NR_VG(ZM, ATTR_TEXC | ATTR_WRAPS)           \
     : mode == (ATTR_TEX_PERSP_BIL | ATTR_WRAPS) ? NR_VG(ZM, ATTR_TEX_PERSP_BIL | ATTR_WRAPS) \
     : mode == (ATTR_TEX_BIL | ATTR_WRAPS) ? NR_VG(ZM, ATTR_TEX_BIL | ATTR_WRAPS)        \
     : mode == (ATTR_TEX_PERSP | ATTR_WRAPS) ? NR_VG(ZM, ATTR_TEX_PERSP | ATTR_WRAPS)    \
     : mode == (ATTR_TEX | ATTR_WRAPS)     ? NR_VG(ZM, ATTR_TEX | ATTR_WRAPS)            \
     : mode == ATTR_TEXC_BIL ? NR_VG(ZM, ATTR_TEXC_BIL)        \
     : mode == ATTR_TEXC    ? NR_VG(ZM, ATTR_TEXC)           \
     : mode == ATTR_TEX_PERSP_BIL ? NR_VG(ZM, ATTR_TEX_PERSP_BIL) \
     : mode == ATTR_TEX_BIL ? NR_VG(ZM, ATTR_TEX_BIL)        \
     : mode == ATTR_TEX_PERSP ? NR_VG(ZM, ATTR_TEX_PERSP)    \
     : mode == ATTR_TEX     ? NR_VG(ZM, ATTR_TEX)            \
     : mode == ATTR_GOURAUD ? NR_VG(ZM, ATTR_GOURAUD)        \
                            : NR_VG(ZM, ATTR_FLAT))
    if (zmode == 1) NR_VZ(1);
    else if (zmode == 2) NR_VZ(2);
    else NR_VZ(0);
#undef NR_VZ
#undef NR_VG
}

}  // namespace nrtri

#if NR_PROBE
extern "C" {
// probe build only: clear / read the k_vis per-item clocks (8 u64 per item)
void NrProbeReset() {
    const unsigned int z = 0;
    NR_CHECK(hipDeviceSynchronize());
    NR_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(nrtri::nr_probe_n), &z, sizeof z));
}
i64 NrProbeRead(unsigned long long* out, i64 maxItems) {
    unsigned int n = 0;
    NR_CHECK(hipDeviceSynchronize());
    NR_CHECK(hipMemcpyFromSymbol(&n, HIP_SYMBOL(nrtri::nr_probe_n), sizeof n));
    const i64 m = std::min<i64>(std::min<i64>((i64)n, maxItems), nrtri::PROBE_MAX);
    NR_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(nrtri::nr_probe_buf), (size_t)m * 8 * sizeof(unsigned long long)));
    return m;
}
}
#endif
