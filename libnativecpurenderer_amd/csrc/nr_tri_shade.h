// nr_tri_shade.h — per-pixel pieces of the order-free raster (nr_free_vis.hip,
// k_vis): the depth of one fragment as a packed visibility key, and the
// deferred shading of a pixel from its winning triangle (record ->
// barycentrics -> colour -> ApplyPixel, cpp:515-549 -> framebuffer, depth and
// frame output).
#pragma once

#include "nr_tri.h"

// Index checks of the shading passes (a build with -DNR_SHADE_CHECK=1 only:
// tools/exp/check.so, loaded with NR_LIB=...): a failed check prints the
// pixel and the indices instead of reading out of range silently.
#ifndef NR_SHADE_CHECK
#define NR_SHADE_CHECK 0
#endif
#if NR_SHADE_CHECK
#define NR_DEV_CHECK(cond, ...)                       \
    do {                                              \
        if (!(cond)) printf("NR_SHADE_CHECK " __VA_ARGS__); \
    } while (0)
#else
#define NR_DEV_CHECK(cond, ...) \
    do {                        \
    } while (0)
#endif

namespace nrtri {

// Doubles of a shading record (build_record): Gouraud sx0 sy0 e1x e1y e2x e2y
// inv | c0 rgb | (c1-c0) rgb | (c2-c0) rgb; flat rgb; textured the same 7
// geometry terms | u0 v0 | (u1-u0) (v1-v0) | (u2-u0) (v2-v0): 13 doubles in
// the Gouraud record's 16-double slot; perspective textured the 7 geometry
// terms | a0 b0 | (a1-a0) (b1-b0) | (a2-a0) (b2-b0) | q0 (q1-q0) (q2-q0) with
// a_k = u_k * q_k, b_k = v_k * q_k: all 16; modulated those 16 | c0 rgb |
// (c1-c0) rgb | (c2-c0) rgb of the corner colours: 25 (an odd stride: the
// records are read as single doubles, 8-byte aligned).  MODE: AttrMode; a
// bilinear mode has no record code of its own -- shade_tile stages its batch
// with the record of its nearest counterpart (attr_unfiltered).
template <int MODE>
struct RecLen {
    static constexpr int REC = attr_modulated(MODE) ? 25 : (MODE != ATTR_FLAT ? 16 : 3);
};

// Depth of a shaded pixel (winner kv; (u32)kv == 0: no fragment won it):
// the winner's depth, or a pending depth clear.
template <int ZMODE>
__device__ __forceinline__ void store_depth(const FrameParams& fp, i64 p, u64 kv) {
    if (ZMODE == 1 && (u32)kv) out_store<u32>(fp.depth + p, (u32)(kv >> 32));
    else if (ZMODE != 0 && fp.pendDepth) out_store<u32>(fp.depth + p, fp.pendDepthValue);
}

// Framebuffer (+ frame output, nr_tri.h store_frame_out) value of pixel p =
// (px, py), written once.
__device__ __forceinline__ void store_colour(const FrameParams& fp, i64 p, i64 px, i64 py, f64 cr, f64 cg, f64 cb,
                                             f64 ca) {
    const int ipp = fp.ipp;
    f64* dst = fp.fb + p * ipp;
    out_store<f64>(dst, cr); out_store<f64>(dst + 1, cg); out_store<f64>(dst + 2, cb);
    if (ipp == 4) out_store<f64>(dst + 3, ca);
    store_frame_out(fp, p, px, py, cr, cg, cb, ca);
}

// ApplyPixel (cpp:529-547) of the winner's colour.  ca == 1 except for
// non-finite barycentrics; the destination is read only then.
__device__ __forceinline__ void apply_winner(const FrameParams& fp, i64 p, f64& cr, f64& cg, f64& cb, f64& ca) {
    cr *= fp.ct[0]; cg *= fp.ct[1]; cb *= fp.ct[2]; ca *= fp.ct[3];
    if (ca != 1) {
        const f64* dst = fp.fb + p * fp.ipp;
        f64 R, G, B;
        if (fp.pendColor) {
            R = G = B = fp.pendColorValue;
        } else {
            R = dst[0]; G = dst[1]; B = dst[2];
        }
        cr = R * (1 - ca) + cr * ca;
        cg = G * (1 - ca) + cg * ca;
        cb = B * (1 - ca) + cb * ca;
    }
}

// Pending clears of a pixel no fragment won.
template <int ZMODE>
__device__ __forceinline__ void store_clear(const FrameParams& fp, i64 p, i64 px, i64 py) {
    if (fp.pendColor) {
        const f64 v = fp.pendColorValue;
        store_colour(fp, p, px, py, v, v, v, v);
    }
    store_depth<ZMODE>(fp, p, 0);
}

// A winner's source data for its shading record: vertices and the rgb of
// each vertex (alpha is not needed, see ShadeStage), loaded as 16 + 8 bytes
// per vertex colour.
template <int MODE>
struct RecordSrc {
    f64 p[MODE != ATTR_FLAT ? 6 : 1];
    // textured: the six uv; perspective textured: the six uv, then the three q; modulated: those nine, then
    // the rgb of each corner
    f64 c[MODE == ATTR_TEXC ? 18 : (MODE == ATTR_GOURAUD || MODE == ATTR_TEX_PERSP ? 9 : (MODE == ATTR_TEX ? 6 : 3))];
};

template <int MODE>
__device__ __forceinline__ void load_record_src(const FrameParams& fp, i64 t, RecordSrc<MODE>& s) {
    constexpr bool GOURAUD = MODE == ATTR_GOURAUD;
    if constexpr (MODE != ATTR_FLAT) load_tri_xy(fp.src.xy, t, s.p);
    if constexpr (MODE == ATTR_TEX) {
        load_tri_xy(fp.src.uv(), t, s.c);   // (the same 3 x 16-byte layout)
        return;
    }
    if constexpr (MODE == ATTR_TEX_PERSP) {
        f64 uv[6];
        load_tri_xy(fp.src.uv(), t, uv);
#pragma unroll
        for (int k = 0; k < 6; ++k) s.c[k] = uv[k];
        const f64* q = fp.q + t * 3;   // (8-byte aligned only: n*3 doubles per batch, like z)
        s.c[6] = q[0]; s.c[7] = q[1]; s.c[8] = q[2];
        return;
    }
    if constexpr (MODE == ATTR_TEXC) {
        f64 a[18];   // per corner (u v | r g | b a)
        load_tri_rgba<18>(fp.src.uvc(), t, a);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.c[2 * k] = a[6 * k]; s.c[2 * k + 1] = a[6 * k + 1];
            s.c[9 + 3 * k] = a[6 * k + 2]; s.c[10 + 3 * k] = a[6 * k + 3]; s.c[11 + 3 * k] = a[6 * k + 4];
        }
        const f64* q = fp.q + t * 3;
        s.c[6] = q[0]; s.c[7] = q[1]; s.c[8] = q[2];
        return;
    }
    const int nv = GOURAUD ? 3 : 1, stride = GOURAUD ? 12 : 4;
#pragma unroll
    for (int v = 0; v < nv; ++v) {
        const f64* q = fp.src.rgba() + t * stride + 4 * v;
        const double2 rg = *reinterpret_cast<const double2*>(q);
        s.c[3 * v] = rg.x; s.c[3 * v + 1] = rg.y; s.c[3 * v + 2] = q[2];
    }
}

// Shading record from its source (the expressions of the per-pixel path, once).
template <int MODE>
__device__ __forceinline__ void build_record(const FrameParams& fp, const RecordSrc<MODE>& s, f64* r) {
    if constexpr (MODE == ATTR_TEX) {
        f64 sx[3], sy[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) nr_xform(fp.m, s.p[2 * v], s.p[2 * v + 1], sx[v], sy[v]);
        const f64 e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
        r[0] = sx[0]; r[1] = sy[0]; r[2] = e1x; r[3] = e1y; r[4] = e2x; r[5] = e2y;
        r[6] = 1.0 / (e1x * e2y - e2x * e1y);
        r[7] = s.c[0]; r[8] = s.c[1];
        r[9] = s.c[2] - s.c[0]; r[10] = s.c[3] - s.c[1];
        r[11] = s.c[4] - s.c[0]; r[12] = s.c[5] - s.c[1];
    } else if constexpr (MODE == ATTR_TEX_PERSP || MODE == ATTR_TEXC) {
        f64 sx[3], sy[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) nr_xform(fp.m, s.p[2 * v], s.p[2 * v + 1], sx[v], sy[v]);
        const f64 e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
        r[0] = sx[0]; r[1] = sy[0]; r[2] = e1x; r[3] = e1y; r[4] = e2x; r[5] = e2y;
        r[6] = 1.0 / (e1x * e2y - e2x * e1y);
        // a_k = u_k * q_k, b_k = v_k * q_k (rounded products), then the differences
        const f64 a0 = s.c[0] * s.c[6], b0 = s.c[1] * s.c[6];
        const f64 a1 = s.c[2] * s.c[7], b1 = s.c[3] * s.c[7];
        const f64 a2 = s.c[4] * s.c[8], b2 = s.c[5] * s.c[8];
        r[7] = a0; r[8] = b0;
        r[9] = a1 - a0; r[10] = b1 - b0;
        r[11] = a2 - a0; r[12] = b2 - b0;
        r[13] = s.c[6]; r[14] = s.c[7] - s.c[6]; r[15] = s.c[8] - s.c[6];
        if constexpr (MODE == ATTR_TEXC) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                r[16 + k] = s.c[9 + k];
                r[19 + k] = s.c[12 + k] - s.c[9 + k];
                r[22 + k] = s.c[15 + k] - s.c[9 + k];
            }
        }
    } else if constexpr (MODE == ATTR_GOURAUD) {
        f64 sx[3], sy[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) nr_xform(fp.m, s.p[2 * v], s.p[2 * v + 1], sx[v], sy[v]);
        const f64 e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
        r[0] = sx[0]; r[1] = sy[0]; r[2] = e1x; r[3] = e1y; r[4] = e2x; r[5] = e2y;
        r[6] = 1.0 / (e1x * e2y - e2x * e1y);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r[7 + k] = s.c[k];
            r[10 + k] = s.c[3 + k] - s.c[k];
            r[13 + k] = s.c[6 + k] - s.c[k];
        }
    } else {
        r[0] = s.c[0]; r[1] = s.c[1]; r[2] = s.c[2];
    }
}

// Shading record of triangle t.
template <int MODE>
__device__ __forceinline__ void make_record(const FrameParams& fp, i64 t, f64* r) {
    RecordSrc<MODE> s;
    load_record_src<MODE>(fp, t, s);
    build_record<MODE>(fp, s, r);
}

// Texture coordinate of pixel (px, py) from a textured record: u and v by the
// expression of a Gouraud channel; from a perspective textured record U, V, Q
// by that expression, then the divide (IEEE) and the two products, u = U * (1 /
// Q), v = V * (1 / Q).  Any Q (zero, negative, non-finite) gives a defined
// texel: the samplers clamp.
template <int MODE>
__device__ __forceinline__ void record_uv(const f64* r, i64 px, i64 py, f64& u, f64& v) {
    const f64 dx = (f64)px - r[0], dy = (f64)py - r[1];
    const f64 w1 = (dx * r[5] - r[4] * dy) * r[6];
    const f64 w2 = (r[2] * dy - dx * r[3]) * r[6];
    u = r[7] + r[9] * w1 + r[11] * w2;
    v = r[8] + r[10] * w1 + r[12] * w2;
    if constexpr (attr_persp(MODE)) {
        const f64 Q = r[13] + r[14] * w1 + r[15] * w2;
        const f64 rq = 1.0 / Q;
        u = u * rq;
        v = v * rq;
    }
}
// Nearest texel (tex_index) of that coordinate.
template <int MODE>
__device__ __forceinline__ i64 record_texel_of(const TexView& tv, const f64* r, i64 px, i64 py) {
    f64 u, v;
    record_uv<MODE>(r, px, py, u, v);
    return tex_index(tv, u, v);
}
// ... under a wrap state (the ATTR_WRAPS instances): tex_index_wrap.
template <int MODE>
__device__ __forceinline__ i64 record_texel_of_wrap(const TexView& tv, const TexWrap& tw, const f64* r, i64 px,
                                                    i64 py) {
    f64 u, v;
    record_uv<MODE>(r, px, py, u, v);
    return tex_index_wrap(tv, tw, u, v);
}

// The four texels of a bilinear footprint at offset ti (tex_bilinear), rgb each: texels (iy, ix) and (iy, ix + 1)
// are adjacent, the second row tv.pitch further.  Ordinary cached loads, like the nearest texel's.
struct TexQuad {
    f64 c[4][3];
};
__device__ __forceinline__ void load_tex_quad(const TexView& tv, i64 ti, TexQuad& t) {
    const f64* q0 = tv.ptr + ti;
    const f64* q1 = q0 + tv.pitch;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.c[0][k] = q0[k]; t.c[1][k] = q0[tv.ipp + k];
        t.c[2][k] = q1[k]; t.c[3][k] = q1[tv.ipp + k];
    }
}
// ... of a wrapped footprint (tex_bilinear_wrap): the +1 column du texels and the +1 row dv texels from the base,
// either way.
__device__ __forceinline__ void load_tex_quad_wrap(const TexView& tv, i64 ti, int du, int dv, TexQuad& t) {
    i64 dcol, drow;
    tex_quad_strides(tv, du, dv, dcol, drow);
    const f64* q0 = tv.ptr + ti;
    const f64* q1 = q0 + drow;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.c[0][k] = q0[k]; t.c[1][k] = q0[dcol + k];
        t.c[2][k] = q1[k]; t.c[3][k] = q1[dcol + k];
    }
}
__device__ __forceinline__ void mix_tex_quad(const TexQuad& t, f64 fu, f64 fv, f64& cr, f64& cg, f64& cb) {
    const f64 gu = 1 - fu, gv = 1 - fv;
    cr = bilinear_mix(t.c[0][0], t.c[1][0], t.c[2][0], t.c[3][0], fu, fv, gu, gv);
    cg = bilinear_mix(t.c[0][1], t.c[1][1], t.c[2][1], t.c[3][1], fu, fv, gu, gv);
    cb = bilinear_mix(t.c[0][2], t.c[1][2], t.c[2][2], t.c[3][2], fu, fv, gu, gv);
}

// A modulated record's interpolated corner colour G at pixel (px, py), times the texel (or filtered) colour in
// cr, cg, cb: one rounded product per channel.  The barycentrics are formed again from the record (the same
// expressions as record_uv, so the same values) rather than kept across the texel gather.  Alpha: the texel's
// literal 1 times 1 + 0*w1 + 0*w2 -- only batches whose every corner alpha is 1, over a texture without alpha,
// are routed to the order-free raster.
__device__ __forceinline__ void record_modulate(const f64* r, i64 px, i64 py, f64& cr, f64& cg, f64& cb, f64& ca) {
    const f64 dx = (f64)px - r[0], dy = (f64)py - r[1];
    const f64 w1 = (dx * r[5] - r[4] * dy) * r[6];
    const f64 w2 = (r[2] * dy - dx * r[3]) * r[6];
    cr = cr * (r[16] + r[19] * w1 + r[22] * w2);
    cg = cg * (r[17] + r[20] * w1 + r[23] * w2);
    cb = cb * (r[18] + r[21] * w1 + r[24] * w2);
    ca = 1.0 * (1.0 + 0.0 * w1 + 0.0 * w2);
}

// Colour of pixel (px, py) from a record.  (Textured: the texel's rgb from
// the view tv, an ordinary cached load -- the filtered rgb of four in a
// bilinear mode; alpha is the literal 1 -- only textures without alpha are
// routed to the order-free raster.)
template <int MODE>
__device__ __forceinline__ void record_colour(const TexView& tv, const f64* r, i64 px, i64 py, f64& cr, f64& cg,
                                              f64& cb, f64& ca) {
    if constexpr (attr_bilinear(MODE)) {
        f64 u, v, fu, fv;
        record_uv<MODE>(r, px, py, u, v);
        TexQuad t;
        load_tex_quad(tv, tex_bilinear(tv, u, v, fu, fv), t);
        mix_tex_quad(t, fu, fv, cr, cg, cb);
        ca = 1.0;
        if constexpr (attr_modulated(MODE)) record_modulate(r, px, py, cr, cg, cb, ca);
    } else if constexpr (attr_textured(MODE)) {
        const f64* q = tv.ptr + record_texel_of<MODE>(tv, r, px, py);
        cr = q[0]; cg = q[1]; cb = q[2]; ca = 1.0;
        if constexpr (attr_modulated(MODE)) record_modulate(r, px, py, cr, cg, cb, ca);
    } else if (MODE == ATTR_GOURAUD) {
        const f64 dx = (f64)px - r[0], dy = (f64)py - r[1];
        const f64 w1 = (dx * r[5] - r[4] * dy) * r[6];
        const f64 w2 = (r[2] * dy - dx * r[3]) * r[6];
        cr = r[7] + r[10] * w1 + r[13] * w2;
        cg = r[8] + r[11] * w1 + r[14] * w2;
        cb = r[9] + r[12] * w1 + r[15] * w2;
        ca = 1.0 + 0.0 * w1 + 0.0 * w2;   // c[3] + (c[7]-c[3])*w1 + (c[11]-c[3])*w2 with unit alphas
    } else {
        cr = r[0]; cg = r[1]; cb = r[2]; ca = 1.0;
    }
}
// ... from a textured record under a wrap state (the ATTR_WRAPS instances): the same with tex_index_wrap /
// tex_bilinear_wrap, the four texels of a footprint by its two signed steps.
template <int MODE>
__device__ __forceinline__ void record_colour_wrap(const TexView& tv, const TexWrap& tw, const f64* r, i64 px, i64 py,
                                                   f64& cr, f64& cg, f64& cb, f64& ca) {
    static_assert(attr_textured(MODE), "textured modes only");
    if constexpr (attr_bilinear(MODE)) {
        f64 u, v, fu, fv;
        int du, dv;
        record_uv<MODE>(r, px, py, u, v);
        TexQuad t;
        const i64 ti = tex_bilinear_wrap(tv, tw, u, v, fu, fv, du, dv);
        load_tex_quad_wrap(tv, ti, du, dv, t);
        mix_tex_quad(t, fu, fv, cr, cg, cb);
    } else {
        const f64* q = tv.ptr + record_texel_of_wrap<MODE>(tv, tw, r, px, py);
        cr = q[0]; cg = q[1]; cb = q[2];
    }
    ca = 1.0;
    if constexpr (attr_modulated(MODE)) record_modulate(r, px, py, cr, cg, cb, ca);
}

// Depth (quantised) of one covered fragment at pixel x = X of a row dy below
// vertex 0 (expressions as the oracle): the per-pixel step of every
// order-free raster.
__device__ __forceinline__ u32 frag_depth(f64 X, f64 dy, f64 sx0, f64 e1x, f64 e1y, f64 e2x, f64 e2y, f64 inv, f64 zz0,
                                          f64 dz1, f64 dz2) {
    const f64 dx = X - sx0;
    const f64 w1 = (dx * e2y - e2x * dy) * inv;
    const f64 w2 = (e1x * dy - dx * e1y) * inv;
    const f64 zz = zz0 + dz1 * w1 + dz2 * w2;
    return nr_quantize_depth_hw(zz);
}
// ... into the tile's LDS keys (k_vis).
template <int ZMODE>
__device__ __forceinline__ void frag_key(u64* key, const u32* zin, int p, f64 X, f64 dy, f64 sx0, f64 e1x, f64 e1y,
                                         f64 e2x, f64 e2y, f64 inv, f64 zz0, f64 dz1, f64 dz2, u64 id1) {
    const u32 zq = frag_depth(X, dy, sx0, e1x, e1y, e2x, e2y, inv, zz0, dz1, dz2);
    if (ZMODE == 1) atomicMin(&key[p], ((u64)zq << 32) | id1);
    else if (zq < zin[p]) atomicMax(&key[p], id1);
}

}  // namespace nrtri
