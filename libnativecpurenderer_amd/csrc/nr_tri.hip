// nr_tri.hip — host API of the triangle / depth / Gouraud path (the
// north-star hot path) and the choice between its two rasterisers:
//   opaque batch (every vertex alpha == 1, colourTransform[3] == 1)
//       -> nr_tri_free.hip    visibility buffer, order-free, load-balanced
//   anything else
//       -> nr_tri_ordered.hip in-order tile raster (blending, painter's order)
// Both produce the oracle's bits; tests/test_parity_gpu.py checks both and
// checks that they agree with each other.
#include "nr_tri.h"

#include <algorithm>
#include <string>
#include <vector>
#include <atomic>
#include <cmath>

namespace nrtri {

bool grow_temp(TriScratch& sc, size_t need) {
    if (need <= sc.temp_bytes && sc.temp) return true;
    if (sc.temp) NR_CHECK(hipFree(sc.temp));
    if (hipMalloc(&sc.temp, need) != hipSuccess) {
        nr_set_error_msg("triangle scratch: hipMalloc failed");
        sc.temp = nullptr;
        sc.temp_bytes = 0;
        return false;
    }
    sc.temp_bytes = need;
    return true;
}

FrameParams frame_params(RenderContext* ctx, const Batch& b) {
    TriScratch& sc = ctx->tri;
    sc.totals();   // (the batch's readbacks use the record: finish_batch, the ordered raster)
    if (ctx->depthTest) nr_ensure_depth(ctx);
    nr_materialize_tiles(ctx, true, true);   // (a batch starts from whole-frame clear state)
    FrameParams fp;
    fp.src = b.src;
    for (int k = 0; k < 6; ++k) fp.m[k] = ctx->m[k];
    for (int k = 0; k < 4; ++k) fp.ct[k] = ctx->ct[k];
    fp.fb = ctx->buffer;
    fp.depth = ctx->depth;
    fp.W = ctx->width;
    fp.H = ctx->height;
    fp.ipp = ctx->enableAlpha ? 4 : 3;
    fp.tiles_x = (int)((ctx->width + TW - 1) / TW);
    fp.tiles_y = (int)((ctx->height + TH - 1) / TH);
    fp.period = ctx->shardPeriod;
    fp.mask = nr_shard_mask(ctx, ctx->shard);
    fp.depthTest = ctx->depthTest;
    fp.depthWrite = ctx->depthWrite;
    fp.pendColor = ctx->pendColor;
    fp.pendColorValue = ctx->pendColorValue;
    fp.pendDepth = ctx->depthTest && ctx->pendDepth;
    fp.pendDepthValue = ctx->pendDepthValue;
    fp.fragCounter = nullptr;
    fp.frameU8 = nullptr;
    fp.frameYUV = ctx->frameFormat == 1;
    fp.tileStamp = nullptr;
    fp.tileEpoch = 0;
    fp.tstamp = nullptr;
    fp.tex = b.tex;
    fp.winMask = nullptr;
    fp.q = b.q;
    fp.wrapU = b.wrap.u;
    fp.wrapV = b.wrap.v;
    if (ctx->countFragments) {
        if (!sc.d_frag) NR_CHECK(hipMalloc(&sc.d_frag, sizeof(u64)));
        NR_CHECK(hipMemsetAsync(sc.d_frag, 0, sizeof(u64), ctx->stream));
        fp.fragCounter = sc.d_frag;
    }
    return fp;
}

// After the raster: account fragments, and mark the deferred clears consumed.
void finish_batch(RenderContext* ctx, const FrameParams& fp) {
    TriScratch& sc = ctx->tri;
    // the u8 mirror is current only when this batch's resolve wrote it for
    // every owned pixel (it does exactly when a clear was pending)
    ctx->frameU8Valid = fp.frameU8 != nullptr;
    if (fp.fragCounter) {
        NR_CHECK(hipMemcpyAsync(&sc.h_total[2], sc.d_frag, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        NR_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->fragTotal += sc.h_total[2];
    }
    if (fp.tileStamp) {   // the empty tiles' clears stay pending (k_vis stamped them)
        ctx->tileColor = fp.pendColor != 0;
        ctx->tileColorValue = fp.pendColorValue;
        ctx->tileDepth = fp.pendDepth != 0;
        ctx->tileDepthValue = fp.pendDepthValue;
    }
    ctx->pendColor = false;
    if (ctx->depthTest) ctx->pendDepth = false;
}

namespace {

// Writes the pending clears of the tiles stamped `epoch` (one workgroup per tile).
__global__ __launch_bounds__(256) void k_tile_clear(f64* __restrict__ fb, u32* __restrict__ depth, i64 W, i64 H,
                                                    int tiles_x, int ipp, const u32* __restrict__ stamp, u32 epoch,
                                                    int doColor, f64 cv, int doDepth, u32 dv) {
    const int tile = blockIdx.x;
    if (stamp[tile] != epoch) return;
    const i64 x0 = (i64)(tile % tiles_x) * TW, y0 = (i64)(tile / tiles_x) * TH;
    for (int p = threadIdx.x; p < TW * TH; p += 256) {
        const i64 px = x0 + (p & (TW - 1)), py = y0 + p / TW;
        if (px >= W || py >= H) continue;
        const i64 q = py * W + px;
        if (doColor)
            for (int c = 0; c < ipp; ++c) fb[q * ipp + c] = cv;
        if (doDepth) depth[q] = dv;
    }
}

}  // namespace

// Stamp array of at least `ntiles` entries (zero = no epoch).
u32* tile_stamps(RenderContext* ctx, i64 ntiles) {
    if (ctx->tileStampCap < ntiles) {
        if (ctx->tileStamp) NR_CHECK(hipFree(ctx->tileStamp));
        NR_CHECK(hipMalloc(&ctx->tileStamp, (size_t)ntiles * sizeof(u32)));
        NR_CHECK(hipMemsetAsync(ctx->tileStamp, 0, (size_t)ntiles * sizeof(u32), ctx->stream));
        ctx->tileStampCap = ntiles;
    }
    if (++ctx->tileEpoch == 0) {   // (wrapped: no stale stamp may equal a new epoch)
        NR_CHECK(hipMemsetAsync(ctx->tileStamp, 0, (size_t)ctx->tileStampCap * sizeof(u32), ctx->stream));
        ctx->tileEpoch = 1;
    }
    return ctx->tileStamp;
}

namespace {

// User-space bounding boxes of the NR_CLUSTER-triangle clusters (TriangleBuffer::cbox).
std::vector<f64> host_cluster_boxes(const f64* xy, i64 n) {
    const i64 nc = (n + NR_CLUSTER - 1) / NR_CLUSTER;
    std::vector<f64> cb((size_t)nc * 4);
    for (i64 c = 0; c < nc; ++c) {
        f64 x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
        bool bad = false;
        for (i64 t = c * NR_CLUSTER; t < std::min<i64>(n, (c + 1) * NR_CLUSTER); ++t)
            for (int v = 0; v < 3; ++v) {
                const f64 x = xy[t * 6 + 2 * v], y = xy[t * 6 + 2 * v + 1];
                if (!std::isfinite(x) || !std::isfinite(y)) bad = true;
                x0 = std::min(x0, x); x1 = std::max(x1, x);
                y0 = std::min(y0, y); y1 = std::max(y1, y);
            }
        if (bad) x0 = y0 = x1 = y1 = NAN;
        cb[c * 4] = x0; cb[c * 4 + 1] = y0; cb[c * 4 + 2] = x1; cb[c * 4 + 3] = y1;
    }
    return cb;
}

Opacity host_opacity(const f64* rgba, i64 n, bool gouraud) {
    const i64 stride = gouraud ? 12 : 4;
    for (i64 t = 0; t < n; ++t)
        for (int v = 0; v < (gouraud ? 3 : 1); ++v)
            if (rgba[t * stride + v * 4 + 3] != 1) return OPQ_BLENDED;
    return OPQ_OPAQUE;
}

// A modulated batch's corner alphas: doubles 5, 11, 17 of each triangle's 18 (u v | r g | b a per corner).
Opacity host_opacity_uvc(const f64* uvc, i64 n) {
    for (i64 t = 0; t < n; ++t)
        for (int v = 0; v < 3; ++v)
            if (uvc[t * 18 + v * 6 + 5] != 1) return OPQ_BLENDED;
    return OPQ_OPAQUE;
}

// Opacity of a device-resident batch the host cannot inspect.
__global__ __launch_bounds__(256) void k_opacity(const f64* __restrict__ rgba, i64 n, int gouraud,
                                                 u32* __restrict__ nonopaque) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t < n) {
        if (gouraud) {
            const f64* a = rgba + t * 12;
            bad = a[3] != 1 || a[7] != 1 || a[11] != 1;
        } else {
            bad = rgba[t * 4 + 3] != 1;
        }
    }
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicOr(nonopaque, 1u);
}

// The same for a modulated batch (a kernel of its own: k_opacity stays as it is).
__global__ __launch_bounds__(256) void k_opacity_uvc(const f64* __restrict__ uvc, i64 n, u32* __restrict__ nonopaque) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t < n) {
        const f64* a = uvc + t * 18;
        bad = a[5] != 1 || a[11] != 1 || a[17] != 1;
    }
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicOr(nonopaque, 1u);
}

Opacity device_opacity(RenderContext* ctx, const TriSrc& src) {
    TriScratch& sc = ctx->tri;
    if (!sc.d_flag) NR_CHECK(hipMalloc(&sc.d_flag, sizeof(u32)));
    NR_CHECK(hipMemsetAsync(sc.d_flag, 0, sizeof(u32), ctx->stream));
    if (attr_modulated(src.mode))
        hipLaunchKernelGGL(k_opacity_uvc, dim3((unsigned)((src.n + 255) / 256)), dim3(256), 0, ctx->stream, src.uvc(),
                           src.n, sc.d_flag);
    else
        hipLaunchKernelGGL(k_opacity, dim3((unsigned)((src.n + 255) / 256)), dim3(256), 0, ctx->stream, src.rgba(),
                           src.n, src.mode == ATTR_GOURAUD ? 1 : 0, sc.d_flag);
    NR_CHECK(hipGetLastError());
    u32* h = reinterpret_cast<u32*>(&sc.totals()[3]);
    NR_CHECK(hipMemcpyAsync(h, sc.d_flag, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
    NR_CHECK(hipStreamSynchronize(ctx->stream));
    return *h ? OPQ_BLENDED : OPQ_OPAQUE;
}

}  // namespace

void draw(RenderContext* ctx, const Batch& b) {
    NR_CHECK(hipSetDevice(ctx->device));
    nr_settle(ctx);   // recorded draws come first (the colour entry points reach here with their list still queued)
    if (b.src.n <= 0 || ctx->width <= 0 || ctx->height <= 0) return;
    if (!ctx->depthTest) nr_materialize_depth(ctx);
    const bool freeEligible = ctx->ct[3] == 1 && ctx->forceOrdered == 0;
    Opacity opq = b.opq;
    if (freeEligible && opq == OPQ_UNKNOWN) opq = device_opacity(ctx, b.src);
    if (freeEligible && opq == OPQ_OPAQUE) draw_free(ctx, b, false);
    else draw_ordered(ctx, b);
}

// A textured batch: the texture is checked (the sampler's clamp to w-2 / h-2
// needs two texels each way), a texture aliasing the target is sampled from a
// snapshot (as DrawTexture), and the batch is opaque exactly when the texture
// has no alpha (every texel's alpha is then 1) -- no scan of the batch.
// Recorded primitive draws run first.  While the batch is pending the texture
// must stay alive as for DrawTexture (DestroyTexture settles every context).
bool check_texture(RenderContext* ctx, const Texture* tex, const char* what) {
    const char* why = nullptr;
    if (!tex || !tex->buffer) why = "NULL texture";
    else if (tex->width < 2 || tex->height < 2) why = "texture narrower or lower than 2 texels";
    else if (tex->width >= (1 << 29) || tex->height >= (1 << 29)) why = "texture side of 2^29 texels or more";
    else if (tex->device != ctx->device) why = "texture on another device";
    if (!why) return true;
    nr_set_error_msg((std::string(what) + ": " + why).c_str());
    return false;
}

// b.q non-null: a perspective textured batch; b.modulated: one whose attributes also carry the corner colours
// (src.attr n*18, b.q required).  The context's filter
// (SetTriangleTextureFilter) is read here, when the draw is issued: the mode is
// part of the batch's snapshot, so a pending batch or its re-run keeps it.  The
// wrap state (SetTriangleTextureWrap) likewise: read here, carried in the batch.
void draw_textured(RenderContext* ctx, Texture* tex, Batch& b) {
    settle(ctx);   // (a re-run of the pending batch comes before a snapshot of the target)
    TexSrc ts = nr_tex_source(ctx, tex);
    b.tex = tex_view(ts.ptr, tex->width, tex->height, tex->enableAlpha);
    b.wrap = tex_wrap(tex->width, tex->height, ctx->texWrapU, ctx->texWrapV);
    if (b.modulated) b.src.mode = ctx->texFilter ? ATTR_TEXC_BIL : ATTR_TEXC;
    else if (ctx->texFilter) b.src.mode = b.q ? ATTR_TEX_PERSP_BIL : ATTR_TEX_BIL;
    else b.src.mode = b.q ? ATTR_TEX_PERSP : ATTR_TEX;
    // (modulated: opaque when also every corner alpha is 1 -- b.opq as the caller found it, or OPQ_UNKNOWN: draw
    // scans the batch on the device, and only when the colour transform and the raster override leave it a choice)
    if (tex->enableAlpha) b.opq = OPQ_BLENDED;
    else if (!b.modulated) b.opq = OPQ_OPAQUE;
    draw(ctx, b);
    if (ts.tmp) {   // (rare: the snapshot must outlive the batch and any re-run of it)
        settle(ctx);
        nr_tex_release(ctx, ts);
    }
}

}  // namespace nrtri

using namespace nrtri;

void nr_materialize_tiles(RenderContext* ctx, bool color, bool depth) {
    nr_deferred_resolve(ctx, color, depth);   // (a deferred batch's cached tiles; the stamped tiles are k_tile_clear's)
    const bool c = color && ctx->tileColor, d = depth && ctx->tileDepth && ctx->depth;
    if (!c && !d) return;
    if (c) ctx->tileColor = false;
    if (d) ctx->tileDepth = false;
    const i64 tx = (ctx->width + TW - 1) / TW, ty = (ctx->height + TH - 1) / TH;
    if (tx * ty <= 0) return;
    hipEvent_t a, b;
    nr_timing_begin(ctx, NRK_FILL, &a, &b);
    hipLaunchKernelGGL(k_tile_clear, dim3((unsigned)(tx * ty)), dim3(256), 0, ctx->stream, ctx->buffer, ctx->depth,
                       ctx->width, ctx->height, (int)tx, ctx->enableAlpha ? 4 : 3, ctx->tileStamp, ctx->tileEpoch,
                       c ? 1 : 0, ctx->tileColorValue, d ? 1 : 0, ctx->tileDepthValue);
    NR_CHECK(hipGetLastError());
    nr_timing_end(ctx, NRK_FILL, a, b);
}

void nr_settle(RenderContext* ctx) {
    nrtri::settle(ctx);
    nr_flush_commands(ctx);   // recorded draws come after the last batch in program order
}

// Stages the soup `s` (s.n > 0, ncol attribute doubles per triangle) for a draw and points `s` at what the batch
// reads; *callerOwned by Batch's rule.  False: the staging array could not be grown (error latched).
//   host arrays: all of them are copied into the context's staging array (TriScratch::stage) -- xy n*6 | z n*3,
//     padded to an even count (keeps the attributes 16-byte aligned) | attributes n*ncol | q n*3 -- and the copy
//     is waited for, so nothing is the caller's afterwards;
//   device arrays: the kernels load positions and attributes as 16-byte vectors, so when xy or the attribute
//     array is not 16-byte aligned those two are re-staged (device-to-device); z and q, read as single
//     doubles, stay the caller's; aligned arrays are used in place.
// The array is overwritten only after settle: a pending batch may still read it.
static bool stage_soup(RenderContext* ctx, Soup& s, size_t ncol, bool onDevice, bool* callerOwned) {
    *callerOwned = onDevice;
    if (onDevice && !(((uintptr_t)s.xy | (uintptr_t)s.attr) & 15)) return true;
    NR_CHECK(hipSetDevice(ctx->device));
    settle(ctx);
    const size_t n = (size_t)s.n, zn = (n * 3 + 1) & ~(size_t)1;
    const bool all = !onDevice;
    if (!ctx->tri.stage.ensure(n * (6 + ncol) + zn + (all && s.q ? n * 3 : 0))) return false;
    f64* const xy = ctx->tri.stage;
    f64* const z = xy + n * 6;
    f64* const attr = z + zn;
    f64* const q = attr + n * ncol;
    const hipMemcpyKind kind = onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    NR_CHECK(hipMemcpyAsync(xy, s.xy, n * 6 * sizeof(f64), kind, ctx->stream));
    if (all && s.z) NR_CHECK(hipMemcpyAsync(z, s.z, n * 3 * sizeof(f64), kind, ctx->stream));
    NR_CHECK(hipMemcpyAsync(attr, s.attr, n * ncol * sizeof(f64), kind, ctx->stream));
    if (all && s.q) NR_CHECK(hipMemcpyAsync(q, s.q, n * 3 * sizeof(f64), kind, ctx->stream));
    if (all) NR_CHECK(hipStreamSynchronize(ctx->stream));   // caller may reuse its arrays on return
    s.xy = xy;
    s.attr = attr;
    if (all && s.z) s.z = z;
    if (all && s.q) s.q = q;
    *callerOwned = onDevice && (s.z || s.q);
    return true;
}

// The six textured soup entry points, under the caller's name `what`; persp: s.q is required; modulated (persp
// too): s.attr is the n*18 uvc array, required.
static void draw_textured_soup(RenderContext* ctx, Texture* tex, Soup s, bool persp, bool onDevice, const char* what,
                               bool modulated = false) {
    NR_CHECK(hipSetDevice(ctx->device));
    nr_settle(ctx);   // a pending batch may still read the staging buffer; recorded draws come first
    if (!check_texture(ctx, tex, what)) return;
    if (modulated && !s.attr) {
        nr_set_error_msg((std::string(what) + ": NULL uvc").c_str());
        return;
    }
    if (persp && !s.q) {
        nr_set_error_msg((std::string(what) + ": NULL q").c_str());
        return;
    }
    if (s.n <= 0) return;
    // (a host soup's corner alphas are looked at only where the answer can matter: draw_textured)
    Opacity opq = OPQ_UNKNOWN;
    if (modulated && !onDevice && !tex->enableAlpha && ctx->ct[3] == 1 && ctx->forceOrdered == 0)
        opq = host_opacity_uvc(s.attr, s.n);
    bool callerOwned;
    if (!stage_soup(ctx, s, modulated ? 18 : 6, onDevice, &callerOwned)) return;
    Batch b = soup_batch(s, ATTR_TEX, opq, nullptr, callerOwned);   // (mode and opacity: draw_textured)
    b.modulated = modulated;
    draw_textured(ctx, tex, b);
}

extern "C" {

// New (no reference counterpart): depth-test LESS on/off, depth write on/off.
void SetDepthState(RenderContext* ctx, bool test, bool write) {
    ctx->depthTest = test;
    ctx->depthWrite = write;
}

// New: the texture filter of this context's textured triangle draws
// (DrawTexturedTriangles and its Device / Perspective variants,
// DrawTexturedTriangleBuffer, DrawTexturedMesh): 0 nearest (the default), 1
// bilinear.  Any other mode latches an error, leaves the state
// unchanged and returns false.  Per context; not part of the save / restore
// stack, not recorded (the mesh states' rule); read when a draw is issued.
// DrawTexture, DrawSplittedTexture and ResampleTexture stay nearest.
bool SetTriangleTextureFilter(RenderContext* ctx, i64 mode) {
    if (mode != 0 && mode != 1) {
        nr_set_error_msg("SetTriangleTextureFilter: mode must be 0 (nearest) or 1 (bilinear)");
        return false;
    }
    ctx->texFilter = (int)mode;
    return true;
}
i64 GetTriangleTextureFilter(RenderContext* ctx) { return ctx->texFilter; }

// New: the wrap addressing of this context's textured triangle draws, per axis
// (everything SetTriangleTextureFilter covers, and the modulated draws): 0 clamp
// (the default), 1 repeat, 2 mirrored repeat.  A mode outside
// 0..2 on either axis latches an error, leaves both axes unchanged and returns
// false.  The filter's rules: per context; not part of the save / restore
// stack, not recorded; read when a draw is issued (draw_textured).
bool SetTriangleTextureWrap(RenderContext* ctx, i64 modeU, i64 modeV) {
    if (modeU < 0 || modeU > 2 || modeV < 0 || modeV > 2) {
        nr_set_error_msg("SetTriangleTextureWrap: modes must be 0 (clamp), 1 (repeat) or 2 (mirror)");
        return false;
    }
    ctx->texWrapU = (int)modeU;
    ctx->texWrapV = (int)modeV;
    return true;
}
void GetTriangleTextureWrap(RenderContext* ctx, i64* modeU, i64* modeV) {
    if (modeU) *modeU = ctx->texWrapU;
    if (modeV) *modeV = ctx->texWrapV;
}

// New: clear the u32 depth buffer (deferred; consumed by the raster).
void ClearDepth(RenderContext* ctx, u32 value) {
    ctx->pendDepth = true;
    ctx->pendDepthValue = value;
    ctx->tileDepth = false;   // (superseded)
    nr_deferred_supersede(ctx, false, true);
}

// New: copy the W*H u32 depth buffer to the host.
void GetDepthBuffer(RenderContext* ctx, u32* out) {
    NR_CHECK(hipSetDevice(ctx->device));
    settle(ctx);
    nr_ensure_depth(ctx);
    nr_materialize_depth(ctx);
    NR_CHECK(hipMemcpyAsync(out, ctx->depth, (size_t)(ctx->width * ctx->height) * sizeof(u32), hipMemcpyDeviceToHost,
                            ctx->stream));
    NR_CHECK(hipStreamSynchronize(ctx->stream));
}

// New: triangles from device-resident arrays (xy n*6, z n*3 or NULL,
// rgba n*4 flat / n*12 Gouraud), in the context's transform.  Asynchronous
// like any kernel launch: the arrays must stay valid and unchanged until the
// batch has executed (Flush, a readback, or any device synchronisation).  The
// visibility path sizes such a batch exactly inside this call (a host wait for
// its binning), so nothing reads the arrays after that point.
void DrawTrianglesDevice(RenderContext* ctx, const f64* xy, const f64* z, const f64* rgba, i64 n, bool gouraud) {
    Soup s{xy, z, rgba, nullptr, n};
    bool callerOwned = true;
    if (n > 0 && !stage_soup(ctx, s, gouraud ? 12 : 4, true, &callerOwned)) return;
    draw(ctx, soup_batch(s, gouraud ? ATTR_GOURAUD : ATTR_FLAT, OPQ_UNKNOWN, nullptr, callerOwned));
}

// New: triangles from host arrays (copied to HBM first).
void DrawTriangles(RenderContext* ctx, const f64* xy, const f64* z, const f64* rgba, i64 n, bool gouraud) {
    NR_CHECK(hipSetDevice(ctx->device));
    settle(ctx);
    if (n <= 0) return;
    Soup s{xy, z, rgba, nullptr, n};
    bool callerOwned;
    if (!stage_soup(ctx, s, gouraud ? 12 : 4, false, &callerOwned)) return;
    draw(ctx, soup_batch(s, gouraud ? ATTR_GOURAUD : ATTR_FLAT, host_opacity(rgba, n, gouraud), nullptr, callerOwned));
}

// New: textured triangles from host arrays (uv: n*6 texel coordinates).
void DrawTexturedTriangles(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uv, i64 n) {
    draw_textured_soup(ctx, tex, Soup{xy, z, uv, nullptr, n}, false, false, "DrawTexturedTriangles");
}

// New: textured triangles from device-resident arrays (as DrawTrianglesDevice).
void DrawTexturedTrianglesDevice(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uv,
                                 i64 n) {
    draw_textured_soup(ctx, tex, Soup{xy, z, uv, nullptr, n}, false, true, "DrawTexturedTrianglesDevice");
}

// New: perspective-correct textured triangles from host arrays (DESIGN.md §3
// "Perspective-correct texture mapping"): q, n*3 laid out like z, is each
// corner's 1/w.  Not validated: any value gives a defined texel.  A NULL q
// latches an error and draws nothing; otherwise as DrawTexturedTriangles.
void DrawTexturedTrianglesPerspective(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uv,
                                      const f64* q, i64 n) {
    draw_textured_soup(ctx, tex, Soup{xy, z, uv, q, n}, true, false, "DrawTexturedTrianglesPerspective");
}

// New: the same from device-resident arrays (as DrawTexturedTrianglesDevice; q
// stays the caller's like z: it is read as single doubles).
void DrawTexturedTrianglesPerspectiveDevice(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z,
                                            const f64* uv, const f64* q, i64 n) {
    draw_textured_soup(ctx, tex, Soup{xy, z, uv, q, n}, true, true, "DrawTexturedTrianglesPerspectiveDevice");
}

// New: modulated textured triangles from host arrays (DESIGN.md §3 "Modulated textured draws"): uvc, n*18, is
// per corner (u, v, r, g, b, a); q as DrawTexturedTrianglesPerspective's (all 1.0 for affine mapping).  The
// fragment's source is the texel at the perspective-correct (u, v), by the context's filter, times the
// interpolated corner colour, channel by channel.  A NULL uvc or a NULL q latches an error and draws nothing;
// otherwise as DrawTexturedTriangles.
void DrawTexturedTrianglesModulated(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uvc,
                                    const f64* q, i64 n) {
    draw_textured_soup(ctx, tex, Soup{xy, z, uvc, q, n}, true, false, "DrawTexturedTrianglesModulated", true);
}

// New: the same from device-resident arrays (DrawTrianglesDevice's rules: xy and uvc are re-staged when not
// 16-byte aligned; z and q stay the caller's).
void DrawTexturedTrianglesModulatedDevice(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z,
                                          const f64* uvc, const f64* q, i64 n) {
    draw_textured_soup(ctx, tex, Soup{xy, z, uvc, q, n}, true, true, "DrawTexturedTrianglesModulatedDevice", true);
}

// New: a device-resident triangle soup (the H2D point; drawn many times).
static TriangleBuffer* create_buffer(i64 n, const f64* xy, const f64* z, const f64* rgba, bool gouraud,
                                     const f64* uv) {
    static std::atomic<u64> g_uid{0};
    TriangleBuffer* tb = new TriangleBuffer();
    tb->uid = ++g_uid;
    tb->n = n;
    tb->gouraud = gouraud;
    tb->textured = uv != nullptr;
    tb->opaque = !uv && n > 0 && host_opacity(rgba, n, gouraud) == OPQ_OPAQUE;
    std::vector<f64> cb;
    if (n > 0) cb = host_cluster_boxes(xy, n);
    NR_CHECK(hipGetDevice(&tb->device));
    hipStream_t s = nr_stream_for(tb->device);
    const size_t ncol = uv ? 6 : (gouraud ? 12 : 4);
    if (n > 0) {
        f64** attr = uv ? &tb->uv : &tb->rgba;
        NR_CHECK(hipMalloc(&tb->xy, (size_t)n * 6 * sizeof(f64)));
        NR_CHECK(hipMalloc(attr, (size_t)n * ncol * sizeof(f64)));
        NR_CHECK(hipMemcpyAsync(tb->xy, xy, (size_t)n * 6 * sizeof(f64), hipMemcpyHostToDevice, s));
        NR_CHECK(hipMemcpyAsync(*attr, uv ? uv : rgba, (size_t)n * ncol * sizeof(f64), hipMemcpyHostToDevice, s));
        if (z) {
            NR_CHECK(hipMalloc(&tb->z, (size_t)n * 3 * sizeof(f64)));
            NR_CHECK(hipMemcpyAsync(tb->z, z, (size_t)n * 3 * sizeof(f64), hipMemcpyHostToDevice, s));
        }
        NR_CHECK(hipMalloc(&tb->cbox, cb.size() * sizeof(f64)));
        NR_CHECK(hipMemcpyAsync(tb->cbox, cb.data(), cb.size() * sizeof(f64), hipMemcpyHostToDevice, s));
        NR_CHECK(hipStreamSynchronize(s));
        f64 b[4] = {INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (size_t c = 0; c + 3 < cb.size(); c += 4) {
            if (std::isnan(cb[c])) { b[0] = b[1] = b[2] = b[3] = NAN; break; }
            b[0] = std::min(b[0], cb[c]); b[1] = std::min(b[1], cb[c + 1]);
            b[2] = std::max(b[2], cb[c + 2]); b[3] = std::max(b[3], cb[c + 3]);
        }
        for (int k = 0; k < 4; ++k) tb->bbox[k] = b[k];
        tb->hcbox = std::move(cb);
    }
    return tb;
}

TriangleBuffer* CreateTriangleBuffer(i64 n, const f64* xy, const f64* z, const f64* rgba, bool gouraud) {
    return create_buffer(n, xy, z, rgba, gouraud, nullptr);
}

// New: a device-resident textured triangle soup (uv: n*6 texel coordinates).
// No texture is bound: DrawTexturedTriangleBuffer names one per draw, and the
// buffer's binning (which reads only xy) stays warm across textures.
TriangleBuffer* CreateTexturedTriangleBuffer(i64 n, const f64* xy, const f64* z, const f64* uv) {
    if (!uv && n > 0) {
        nr_set_error_msg("CreateTexturedTriangleBuffer: NULL uv");
        return nullptr;
    }
    static const f64 none[6] = {0, 0, 0, 0, 0, 0};
    return create_buffer(n, xy, z, nullptr, false, uv ? uv : none);
}

void DestroyTriangleBuffer(TriangleBuffer* tb) {
    if (!tb) return;
    // a context's pending batch may reference tb: the stream sync below
    // completes it; an overflow re-run would need tb, so settle all first
    nr_settle_all();
    nr_deferred_resolve_buffer(tb);   // (pending values are formed from tb's arrays: written before the frees)
    NR_CHECK(hipSetDevice(tb->device));
    NR_CHECK(hipStreamSynchronize(nr_stream_for(tb->device)));
    NR_CHECK(hipStreamSynchronize(nr_bin_stream_for(tb->device)));
    if (tb->xy) NR_CHECK(hipFree(tb->xy));
    if (tb->z) NR_CHECK(hipFree(tb->z));
    if (tb->rgba) NR_CHECK(hipFree(tb->rgba));
    if (tb->uv) NR_CHECK(hipFree(tb->uv));
    if (tb->cbox) NR_CHECK(hipFree(tb->cbox));
    delete tb;
}

i64 GetTriangleBufferCount(TriangleBuffer* tb) { return tb->n; }

void DrawTriangleBuffer(RenderContext* ctx, TriangleBuffer* tb) {
    if (tb->textured) {
        nr_set_error_msg("DrawTriangleBuffer: a textured buffer (use DrawTexturedTriangleBuffer)");
        return;
    }
    // a TriangleBuffer never changes: its binning may overlap the previous batch's raster
    draw(ctx, soup_batch(Soup{tb->xy, tb->z, tb->rgba, nullptr, tb->n}, tb->gouraud ? ATTR_GOURAUD : ATTR_FLAT,
                         tb->opaque ? OPQ_OPAQUE : OPQ_BLENDED, tb, false));
}

// New: a textured TriangleBuffer sampled from `tex` (chosen per draw).
void DrawTexturedTriangleBuffer(RenderContext* ctx, TriangleBuffer* tb, Texture* tex) {
    NR_CHECK(hipSetDevice(ctx->device));
    if (!tb || !tb->textured) {
        nr_set_error_msg("DrawTexturedTriangleBuffer: not a textured buffer (use DrawTriangleBuffer)");
        return;
    }
    if (ctx->recording) nr_settle(ctx);   // recorded draws come first
    if (!check_texture(ctx, tex, "DrawTexturedTriangleBuffer")) return;
    Batch b = soup_batch(Soup{tb->xy, tb->z, tb->uv, nullptr, tb->n}, ATTR_TEX, OPQ_UNKNOWN, tb, false);
    draw_textured(ctx, tex, b);
}

// New: count covered on-screen pixel x triangle pairs (the "shaded+Z-tested
// fragments" work count of the Mpixels/s metric).  Counting uses a separate
// kernel variant and syncs per draw: enable it outside timed regions.
void SetFragmentCounting(RenderContext* ctx, bool on) {
    ctx->countFragments = on;
    ctx->fragTotal = 0;
}
i64 GetFragmentCount(RenderContext* ctx) { return (i64)ctx->fragTotal; }

// New (testing / A-B measurement): warm binning of a TriangleBuffer drawn
// again under the key of its last validated binning (one binning pass into
// the kept tile ranges), 0 automatic (NR_WARM), 1 on, 2 off.
void SetWarmBinning(RenderContext* ctx, i64 mode) {
    ctx->tri.warmMode = (int)(mode >= 0 && mode <= 2 ? mode : 0);
    if (ctx->tri.warmMode == 2) {   // (no kept pair list, and no visible list, outlives the switch)
        ctx->tri.sched.listSet = -1;
        ctx->tri.sched.drop_visible();
    }
}
// New (testing): number of batches of this context binned warm so far.
i64 GetWarmBatchCount(RenderContext* ctx) { return (i64)ctx->tri.warmBatches; }
// New (testing): of those, batches binned into the loose ranges (a changed transform).
i64 GetLooseBatchCount(RenderContext* ctx) { return (i64)ctx->tri.looseBatches; }
// New (testing): of the warm batches, those rasterised from the pair list an
// earlier warm batch under the same key left in place (no binning at all).
i64 GetReusedBatchCount(RenderContext* ctx) { return (i64)ctx->tri.reusedBatches; }
// New (testing / A-B measurement): list reuse, 0 automatic (on), 2 off (every
// warm batch bins, the cursors running on from epoch to epoch).
void SetListReuse(RenderContext* ctx, i64 mode) { ctx->tri.reuseMode = mode == 2 ? 2 : 0; }
// New (testing): of the reused batches, those rasterised from the schedule's
// visible list (the kept pair list without the triangles that win no pixel).
i64 GetPrunedBatchCount(RenderContext* ctx) { return (i64)ctx->tri.prunedBatches; }
// New (testing): pairs kept in the current visible list, 0 when there is none.
i64 GetVisiblePairCount(RenderContext* ctx) {
    NR_CHECK(hipSetDevice(ctx->device));
    return nrtri::visible_pairs(ctx);
}
// New (testing / A-B measurement): the visible list, 0 automatic (on), 2 off
// (reused batches rasterise from the full list; a list already pruned is kept
// and used again after a switch back to 0).
void SetVisiblePruning(RenderContext* ctx, i64 mode) { ctx->tri.pruneMode = mode == 2 ? 2 : 0; }
// New (testing / A-B measurement): the visible plan -- the pruned list's own
// work items, planned from the kept counts -- 0 automatic (on), 2 off (pruned
// batches run the schedule's items over the pruned list in place).
void SetVisibleReplan(RenderContext* ctx, i64 mode) { ctx->tri.replanMode = mode == 2 ? 2 : 0; }
// New (testing): of the pruned batches, those rasterised under the visible plan.
i64 GetReplannedBatchCount(RenderContext* ctx) { return (i64)ctx->tri.replannedBatches; }
// New (testing): totals of the current visible plan -- out[0..3] = kept pairs,
// k_vis work items, slices of split tiles, dense tiles; false (and zeros) when
// there is none.  Waits for the device.
bool GetVisiblePlanTotals(RenderContext* ctx, i64* out) {
    NR_CHECK(hipSetDevice(ctx->device));
    return nrtri::visible_plan_totals(ctx, out);
}
// New (testing / A-B measurement): the key cache -- an unchanged draw shaded
// from the final visibility keys one capture frame stored, no raster -- 0
// automatic (on), 2 off (such draws run from the visible list; the cached keys
// are kept and used again after a switch back to 0).
void SetKeyCache(RenderContext* ctx, i64 mode) { ctx->tri.keyMode = mode == 2 ? 2 : 0; }
// New (testing): of the pruned batches, those shaded from the key cache.
i64 GetKeyCachedBatchCount(RenderContext* ctx) { return (i64)ctx->tri.keyCachedBatches; }
// New (testing): totals of the current key cache -- out[0..2] = cached tiles,
// key items (one per owned tile), bytes of cached keys; false (and zeros) when
// there is none.  Waits for the device.
bool GetKeyCacheTotals(RenderContext* ctx, i64* out) {
    NR_CHECK(hipSetDevice(ctx->device));
    return nrtri::key_cache_totals(ctx, out);
}
// New (testing / A-B measurement): the key index -- a cached Gouraud draw shaded
// from the per-tile winner index built with the capture frame (k_keys_idx) -- 0
// automatic (on), 2 off (such draws run k_keys; the index is kept and used again
// at once after a switch back to 0).
void SetKeyIndex(RenderContext* ctx, i64 mode) { ctx->tri.keyIndexMode = mode == 2 ? 2 : 0; }
// New (testing): of the cached batches, those shaded from the key index.
i64 GetKeyIndexedBatchCount(RenderContext* ctx) { return (i64)ctx->tri.keyIndexedBatches; }
// New (testing): totals of the current key index -- out[0..3] = indexed tiles,
// staged winners (the sum of the tiles' counts), pixels whose winner is not
// staged, bytes of the index; false (and zeros) while the generation has none.
// Waits for the device.
bool GetKeyIndexTotals(RenderContext* ctx, i64* out) {
    NR_CHECK(hipSetDevice(ctx->device));
    return nrtri::key_index_totals(ctx, out);
}
// New (testing / A-B measurement): the key records -- an indexed Gouraud draw shaded from the winners' shading
// records, built once per generation (k_keys_rec) -- 0 automatic (on), 2 off (such draws run k_keys_idx; the
// records are kept and used again at once after a switch back to 0).
void SetKeyRecords(RenderContext* ctx, i64 mode) { ctx->tri.keyRecordMode = mode == 2 ? 2 : 0; }
// New (testing): of the indexed batches, those shaded from the key records.
i64 GetKeyRecordBatchCount(RenderContext* ctx) { return (i64)ctx->tri.keyRecordBatches; }
// New (testing): totals of the current key records -- out[0..2] = slots, records (the sum of the tiles' distinct
// winners), bytes of records; false (and zeros) while the generation has none.  Waits for the device.
bool GetKeyRecordTotals(RenderContext* ctx, i64* out) {
    NR_CHECK(hipSetDevice(ctx->device));
    return nrtri::key_record_totals(ctx, out);
}
// New: deferred stores -- a cached Gouraud draw that writes the frame output itself leaves the cached tiles' f64
// framebuffer values and depths pending until something uses the buffers -- 0 automatic (the rule
// of nr_defer_policy.h: only after records in a row that nothing needed), 1 always (every eligible batch; tests
// and A/B), 2 off.  Switching never touches a live record.
void SetDeferredStores(RenderContext* ctx, i64 mode) { ctx->tri.deferMode = (int)(mode >= 0 && mode <= 2 ? mode : 0); }
// New (testing): out[0..3] = batches that deferred, resolve kernels launched, records that ended superseded
// (their values never needed), the rule's current threshold.  Host state: does not wait for the device.
void GetDeferredStoreCounts(RenderContext* ctx, i64* out) {
    const TriScratch& sc = ctx->tri;
    out[0] = (i64)sc.deferredBatches; out[1] = (i64)sc.deferResolves; out[2] = (i64)sc.deferSuperseded;
    out[3] = (i64)sc.deferPolicy.threshold;
}
// New (testing): totals of the context's warm schedule -- out[0..3] = (tile,
// triangle) pairs, k_vis work items, slices of split tiles, dense tiles;
// false (and zeros) when it has none.
bool GetScheduleTotals(RenderContext* ctx, i64* out) {
    NR_CHECK(hipSetDevice(ctx->device));
    nrtri::settle(ctx);
    const auto& S = ctx->tri.sched;
    const BatchTotals t = S.valid ? S.totals : BatchTotals{};
    out[0] = t.pairs; out[1] = t.items; out[2] = t.split; out[3] = t.heavy;
    return S.valid;
}
// New (testing): a fault in the next warm batch -- 1 its binning finds its
// tiles over their ranges, 2 (a batch binned beside the raster) its token is
// withheld (the raster's wait times out after 1 s), 3 it drops a workgroup's
// pairs, 4 (beside the raster) its binning is held back 1.5 s, so that it
// lands after the raster's fallback.  The raster must then run its fallback (k_vis WarmCheck): the frame
// stays exact and the failure is latched (GetWarmFailureCount, the error).
void SetWarmFaultInjection(RenderContext* ctx, i64 mode) { ctx->tri.warmInject = (int)(mode >= 0 && mode <= 4 ? mode : 0); }
// New (testing): warm batches whose checks failed so far (read at API calls).
i64 GetWarmFailureCount(RenderContext* ctx) {
    NR_CHECK(hipSetDevice(ctx->device));
    nrtri::settle(ctx);
    return (i64)ctx->tri.warmFailures;
}

// New: which raster the last batch took (1 = order-free tiled, 2 = ordered).
i64 GetLastRasterPath(RenderContext* ctx) { return ctx->lastPath; }

// New (testing): cap the visibility path's pair list (0 = automatic), to
// exercise the overflow re-run of nr_settle.
void SetPairCapacityOverride(RenderContext* ctx, i64 pairs) {
    ctx->tri.capOverride = (u64)(pairs > 0 ? pairs : 0);
    if (ctx->tri.capOverride) {
        ctx->tri.sched.listSet = -1;
        ctx->tri.sched.drop_visible();
    }
}

// New (testing / A-B measurement): force the ordered raster for every batch.
void SetForceOrderedRaster(RenderContext* ctx, bool on) { ctx->forceOrdered = on ? 1 : 0; }

// New (testing / A-B measurement): k_vis variant, 0 automatic (previous
// batch's pair density), 1 with the wave-cooperative pass for large
// triangles, 2 without it.
void SetCoopRaster(RenderContext* ctx, i64 mode) { ctx->tri.coopMode = (int)(mode >= 0 && mode <= 2 ? mode : 0); }
// NEW (testing / tuning): a tile of more than min(slice, splitAt) pairs is split
// into slices of about dslice pairs (k_vis); 0 restores the defaults.
void SetSplitLimits(RenderContext* ctx, i64 splitAt, i64 dslice) {
    ctx->tri.splitAt = (u32)(splitAt > 0 ? splitAt : 0);
    ctx->tri.dslice = (u32)(dslice > 0 ? dslice : 0);
}

}  // extern "C"
