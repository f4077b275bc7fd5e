// nr_tri.h — shared pieces of the triangle / depth / Gouraud path.
//
// Semantics (no reference implementation exists; defined
// in the reference's idiom, DESIGN.md §3, restated by the CPU oracle):
//   vertices -> context transform (cpp:446-453) -> screen space;
//   coverage = even-odd pointInPolygon (cpp:822-845) at integer pixels;
//   w1,w2 barycentric in f64, attr = a0 + (a1-a0)*w1 + (a2-a0)*w2 (a colour
//   channel, or a texture coordinate whose texel is then the colour; a
//   perspective textured batch interpolates u q, v q and q that way and
//   samples at (U * (1 / Q), V * (1 / Q)); a modulated batch does that and
//   also interpolates a colour G per corner that way: src_c = T_c * G_c, the
//   texel times the colour, one rounded product per channel r, g, b, A -- the
//   alpha of a texture without alpha the literal 1.0);
//   depth u32 LESS, written only when test+write are on;
//   blend = ApplyPixel (cpp:515-549) in submission order.
//
// Two rasterisers share the screen tiling (64x32 tiles) and these helpers:
//   nr_tri_ordered.hip  in-order tile raster (any batch: blending, Z w/o write)
//   nr_tri_free.hip     visibility-buffer raster (opaque batches: every
//                       fragment overwrites, so per-pixel results are an
//                       order-independent min/max over packed keys); its
//                       kernels are in nr_free_bin.hip and nr_free_vis.hip
#pragma once

#include "nr_common.h"

namespace nrtri {

constexpr int TW = 64;   // tile width  (= one wave's lanes)
constexpr int TH = 32;   // tile height

// Per-triangle attribute of a batch: one colour, a colour per vertex, or a
// texture coordinate per vertex (texel units) sampled from FrameParams::tex --
// interpolated affinely in screen space (ATTR_TEX), or perspective-correct
// with a 1/w per vertex, FrameParams::q (ATTR_TEX_PERSP).  The
// two _BIL modes are those two with the bilinear filter (SetTriangleTextureFilter,
// tex_bilinear) in place of the nearest texel: the same batch, record and
// coordinates, four texels per fragment.  The two modulated modes (ATTR_TEXC nearest, ATTR_TEXC_BIL
// bilinear; DESIGN.md §3 "Modulated textured draws") are perspective textured batches that also carry a
// colour per corner: the fragment's source is the texel times the interpolated colour, channel by channel.
enum AttrMode {
    ATTR_FLAT = 0, ATTR_GOURAUD = 1, ATTR_TEX = 2, ATTR_TEX_PERSP = 3, ATTR_TEX_BIL = 4, ATTR_TEX_PERSP_BIL = 5,
    ATTR_TEXC = 6, ATTR_TEXC_BIL = 7
};
// any textured mode: the colour is a texel (or four, filtered); the attribute array holds the uv -- alone
// (n*6), or in a modulated mode interleaved with the corner colours (n*18)
__host__ __device__ constexpr bool attr_textured(int mode) { return mode >= ATTR_TEX && mode <= ATTR_TEXC_BIL; }
// texel times interpolated vertex colour
__host__ __device__ constexpr bool attr_modulated(int mode) { return mode == ATTR_TEXC || mode == ATTR_TEXC_BIL; }
__host__ __device__ constexpr bool attr_persp(int mode) {
    return mode == ATTR_TEX_PERSP || mode == ATTR_TEX_PERSP_BIL || attr_modulated(mode);
}
__host__ __device__ constexpr bool attr_bilinear(int mode) {
    return mode == ATTR_TEX_BIL || mode == ATTR_TEX_PERSP_BIL || mode == ATTR_TEXC_BIL;
}
// the nearest mode whose per-triangle data (record, setup slots) a textured mode shares
__host__ __device__ constexpr int attr_unfiltered(int mode) {
    return mode == ATTR_TEX_BIL ? ATTR_TEX
           : (mode == ATTR_TEX_PERSP_BIL ? ATTR_TEX_PERSP : (mode == ATTR_TEXC_BIL ? ATTR_TEXC : mode));
}

struct TriSrc {
    const f64* xy;    // n*6
    const f64* z;     // n*3 or null
    const f64* attr;  // by mode: colours n*4 flat / n*12 Gouraud, uv n*6 textured (u0 v0 u1 v1 u2 v2), or
                      // n*18 modulated: per corner (u v | r g | b a), three 16-byte words
    int mode;         // AttrMode
    i64 n;
    __host__ __device__ const f64* rgba() const { return attr; }   // (flat / Gouraud batches)
    __host__ __device__ const f64* uv() const { return attr; }     // (textured batches that are not modulated)
    __host__ __device__ const f64* uvc() const { return attr; }    // (modulated batches)
};
// doubles of the attribute array per triangle
__host__ __device__ inline int attr_stride(int mode) {
    return mode == ATTR_GOURAUD ? 12 : (attr_modulated(mode) ? 18 : (attr_textured(mode) ? 6 : 4));
}

// The texture a textured batch samples (tex_index, tex_bilinear): texels as the
// framebuffer stores them, ipp doubles each, w >= 2 and h >= 2 (a side below
// 2^29, so the pitch fits an int: check_texture).  The sampler's clamp bounds (f64)(w-2), (f64)(h-2)
// are formed on the host -- the same values -- so that they arrive as scalar
// kernel arguments: converted in the kernel they are loop-invariant vector
// values, which the compiler hoists and keeps live (or spills) across the
// whole raster; the view is 8 scalar registers.
struct TexView {
    const f64* ptr;
    f64 xlast, ylast;   // w-2, h-2
    int pitch, ipp;     // doubles per row / per texel
};
inline TexView tex_view(const f64* ptr, i64 w, i64 h, bool alpha) {
    const int ipp = alpha ? 4 : 3;
    return TexView{ptr, (f64)(w - 2), (f64)(h - 2), (int)w * ipp, ipp};
}

// The wrap addressing of a textured batch (SetTriangleTextureWrap), per axis: mode 0 clamp (tex_index /
// tex_bilinear on that axis), 1 repeat, 2 mirrored repeat (wrap_fold).  Run-time data of the batch, not an AttrMode:
// one int per axis, mode | side << 2 (a side is below 2^29), formed on the host.  They arrive as scalar kernel
// arguments, so an axis's mode is a wave-uniform scalar branch, and everything the fold needs of them -- the side,
// the period and the period as an f64 (wrap_period) -- is formed by scalar integer operations (an int converted to
// f64 in the kernel is a loop-invariant vector value: see TexView).  Only a batch with a wrapped axis (any()) runs
// the instances that read them (ATTR_WRAPS, below); a (0, 0) batch runs the instances that know no wrap state.
struct TexWrap {
    int u, v;   // columns (side w), rows (side h)
    __host__ __device__ bool any() const { return ((u | v) & 3) != 0; }
};
inline TexWrap tex_wrap(i64 w, i64 h, int mu, int mv) { return TexWrap{mu | (int)(w << 2), mv | (int)(h << 2)}; }
// The rasters' kernels are instantiated per AttrMode.  A textured mode has two instances: the one for batches whose
// state is (0, 0), whose samplers and code are what they were before there was a wrap state, and one for batches
// with a wrapped axis, named by this flag beside the AttrMode in the kernel's mode parameter (a flag in that int,
// not a further template parameter: the symbols of the existing instances stay what they were).  It is no batch
// mode: TriSrc::mode never carries it; the host adds it at the launch when TexWrap::any().
constexpr int ATTR_WRAPS = 8;
__host__ __device__ constexpr int attr_base(int modew) { return modew & (ATTR_WRAPS - 1); }
__host__ __device__ constexpr bool attr_wraps(int modew) { return (modew & ATTR_WRAPS) != 0; }

struct BinParams {
    TriSrc src;
    f64 m[6];
    i64 W, H;
    int tiles_x;
    int period;           // owned tile rows: bit (ty % period) of mask (SetShard / SetShardSlots)
    u64 mask;
    // the owned tile rows, numbered 0.. (the binning kernels' LDS histograms
    // hold only those): pc owned slots per period, slotOf[k] = the k-th
    // owned slot; hrows = owned rows of the frame (set_owned_rows)
    int pc, hrows;
    unsigned char slotOf[64];
};

// Ordinal of owned tile row ty among the owned rows, and its inverse
// (unsharded: the identity, no division).
__device__ __forceinline__ int owned_ord(const BinParams& bp, int ty) {
    if (bp.period == 1) return ty;
    const int q = ty / bp.period, s = ty - q * bp.period;
    return q * bp.pc + __builtin_popcountll(bp.mask & ((1ull << s) - 1ull));
}
__device__ __forceinline__ int owned_row_of(const BinParams& bp, int ord) {
    if (bp.period == 1) return ord;
    const int q = ord / bp.pc;
    return q * bp.period + bp.slotOf[ord - q * bp.pc];
}
inline void set_owned_rows(BinParams& bp, int tiles_y) {
    bp.pc = 0;
    for (int s = 0; s < bp.period && s < 64; ++s)
        if ((bp.mask >> s) & 1ull) bp.slotOf[bp.pc++] = (unsigned char)s;
    bp.hrows = 0;
    for (int ty = 0; ty < tiles_y; ++ty)
        if (bp.period == 1 || ((bp.mask >> (ty % bp.period)) & 1ull)) ++bp.hrows;
}

// (unsharded: no integer division -- it costs ~30 VALU instructions)
__host__ __device__ __forceinline__ bool owned_row(int ty, int period, u64 mask) {
    return period == 1 || ((mask >> (ty % period)) & 1ull);
}

__device__ __forceinline__ f64 clampd(f64 v, f64 lo, f64 hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Triangle arrays are 16-byte aligned (hipMalloc'd, or staged by the draw
// entry points): a triangle's 6 positions / 12 or 4 colours load as 16-byte
// vectors, 3 or 6 or 2 loads instead of 6 or 12 or 4.
__device__ __forceinline__ void load_tri_xy(const f64* xy, i64 t, f64 (&v)[6]) {
    const double2* q = reinterpret_cast<const double2*>(xy + t * 6);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double2 a = q[k];
        v[2 * k] = a.x; v[2 * k + 1] = a.y;
    }
}

template <int N>   // 4 (flat), 12 (Gouraud) or 18 (modulated: uv and colour interleaved)
__device__ __forceinline__ void load_tri_rgba(const f64* rgba, i64 t, f64 (&c)[N]) {
    const double2* q = reinterpret_cast<const double2*>(rgba + t * N);
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        const double2 a = q[k];
        c[2 * k] = a.x; c[2 * k + 1] = a.y;
    }
}

// Screen-space vertices of triangle t (cpp:446-453 applied to each vertex).
__device__ __forceinline__ void tri_screen(const TriSrc& s, const f64* m, i64 t, f64 (&sx)[3], f64 (&sy)[3]) {
    f64 p[6];
    load_tri_xy(s.xy, t, p);
#pragma unroll
    for (int v = 0; v < 3; ++v) nr_xform(m, p[2 * v], p[2 * v + 1], sx[v], sy[v]);
}

__device__ __forceinline__ bool tri_finite(const f64 (&sx)[3], const f64 (&sy)[3]) {
    return isfinite(sx[0]) && isfinite(sy[0]) && isfinite(sx[1]) && isfinite(sy[1]) && isfinite(sx[2]) &&
           isfinite(sy[2]);
}

// Tile rectangle touched by a triangle; false if it produces no fragment.
// Rows: a row y has a straddling edge iff ymin <= y < ymax (exact), so
// [ceil(ymin), ceil(ymax)).  Columns: crossings lie in [xmin, xmax] up to
// rounding, so [floor(xmin)-2, ceil(xmax)+2]; for |coord| > 1e7 the full width.
__device__ __forceinline__ bool tri_tiles(const f64 (&sx)[3], const f64 (&sy)[3], i64 W, i64 H, int& tx0, int& tx1,
                                          int& ty0, int& ty1) {
    bool huge = false;
#pragma unroll
    for (int v = 0; v < 3; ++v) huge = huge || fabs(sx[v]) > 1e7 || fabs(sy[v]) > 1e7;
    if (!tri_finite(sx, sy)) return false;
    const f64 e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
    const f64 den = e1x * e2y - e2x * e1y;
    if (den == 0) return false;
    const f64 ymn = fmin(fmin(sy[0], sy[1]), sy[2]), ymx = fmax(fmax(sy[0], sy[1]), sy[2]);
    const i64 r0 = (i64)clampd(ceil(ymn), 0.0, (f64)H);
    const i64 r1 = (i64)clampd(ceil(ymx), 0.0, (f64)H);
    if (r0 >= r1) return false;
    i64 c0 = 0, c1 = W - 1;
    if (!huge) {
        const f64 xmn = fmin(fmin(sx[0], sx[1]), sx[2]), xmx = fmax(fmax(sx[0], sx[1]), sx[2]);
        if (ceil(xmx) + 2 < 0 || floor(xmn) - 2 > (f64)(W - 1)) return false;
        c0 = (i64)clampd(floor(xmn) - 2, 0.0, (f64)(W - 1));
        c1 = (i64)clampd(ceil(xmx) + 2, 0.0, (f64)(W - 1));
    }
    tx0 = (int)(c0 / TW); tx1 = (int)(c1 / TW);
    ty0 = (int)(r0 / TH); ty1 = (int)((r1 - 1) / TH);
    return true;
}

// Exact covered columns [xs, xe) of screen row y, relative to x0 and clamped
// to [0, wlim].  The two edges straddling y (pointInPolygon's edge order
// (i=0,j=2) (i=1,j=0) (i=2,j=1) and crossing expression, cpp:832-839) give
// crossings ca, cb; (x < ca) != (x < cb)  <=>  ceil(min) <= x < ceil(max).
__device__ __forceinline__ void row_span(const f64 (&sx)[3], const f64 (&sy)[3], f64 y, f64 x0, f64 wlim, int& xs,
                                         int& xe) {
    f64 c0 = 0, c1 = 0;
    int nc = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 2) % 3;
        if ((sy[i] > y) != (sy[j] > y)) {
            const f64 cc = (sx[j] - sx[i]) * (y - sy[i]) / (sy[j] - sy[i]) + sx[i];
            if (nc == 0) c0 = cc; else c1 = cc;
            ++nc;
        }
    }
    xs = xe = 0;
    if (nc == 2) {
        const f64 lo = fmin(c0, c1), hi = fmax(c0, c1);
        xs = (int)clampd(ceil(lo) - x0, 0.0, wlim);
        xe = (int)clampd(ceil(hi) - x0, 0.0, wlim);
        if (xe < xs) xe = xs;
    }
}

// row_span for a row known to lie in [ceil(ymin), ceil(ymax)) (ymin <= y <
// ymax), without branches.  There exactly one vertex v is on its own side of
// y (sy[v] > y differs from the other two), and the two straddling edges are
// the two edges at v; in pointInPolygon's (i, j) orientation those are
// v=0: (0,2) (1,0)   v=1: (2,1) (1,0)   v=2: (0,2) (2,1).
// The crossings are evaluated with the same expression, and min/max does not
// depend on which edge comes first, so the span equals row_span's.
__device__ __forceinline__ void row_span_in(const f64 (&sx)[3], const f64 (&sy)[3], f64 y, f64 x0, f64 wlim,
                                            int& xs, int& xe) {
    const bool b0 = sy[0] > y, b1 = sy[1] > y, b2 = sy[2] > y;
    const bool v1 = (b1 != b0) && (b1 != b2);
    const bool v2 = (b2 != b0) && (b2 != b1);
    // edge A: v==1 ? (2,1) : (0,2);  edge B: v==2 ? (2,1) : (1,0)
    const f64 aix = v1 ? sx[2] : sx[0], aiy = v1 ? sy[2] : sy[0];
    const f64 ajx = v1 ? sx[1] : sx[2], ajy = v1 ? sy[1] : sy[2];
    const f64 bix = v2 ? sx[2] : sx[1], biy = v2 ? sy[2] : sy[1];
    const f64 bjx = v2 ? sx[1] : sx[0], bjy = v2 ? sy[1] : sy[0];
    const f64 ca = (ajx - aix) * (y - aiy) / (ajy - aiy) + aix;
    const f64 cb = (bjx - bix) * (y - biy) / (bjy - biy) + bix;
    const f64 lo = fmin(ca, cb), hi = fmax(ca, cb);
    xs = (int)clampd(ceil(lo) - x0, 0.0, wlim);
    xe = (int)clampd(ceil(hi) - x0, 0.0, wlim);
    if (xe < xs) xe = xs;
}

// Edge slopes for row_span_slopes, one per pointInPolygon edge (i, j) in its
// orientation: e0 = (0,2), e1 = (1,0), e2 = (2,1); slope = (sx[j]-sx[i]) /
// (sy[j]-sy[i]) (inf/NaN for a horizontal edge, which never straddles a row).
__device__ __forceinline__ void edge_slopes(const f64 (&sx)[3], const f64 (&sy)[3], f64 (&sl)[3]) {
    sl[0] = (sx[2] - sx[0]) / (sy[2] - sy[0]);
    sl[1] = (sx[0] - sx[1]) / (sy[0] - sy[1]);
    sl[2] = (sx[1] - sx[2]) / (sy[1] - sy[2]);
}

// One crossing without a division.  The exact crossing is
//   cc  = fl(fl(fl(a*b) / d) + c)      a = sx[j]-sx[i], b = y-sy[i], d = sy[j]-sy[i], c = sx[i]
// and with the per-edge slope s = fl(a/d):
//   cc' = fl(fl(b*s) + c).
// With unit roundoff u = 2^-53 both products are A(1+e)(1+e') for A = a*b/d,
// so |fl(a*b)/d - fl(b*s)| <= (4u + 2u^2)|A|, and the two final roundings add
// u|cc| + u|cc'|; hence |cc - cc'| <= 4.001u|v| + 2.001u|cc'| (v = fl(b*s))
// < 2^-50 (|v| + |cc'|) = eps (plus 2^-1000 for underflow).  ceil is what the
// span needs: if cc' is more than eps away from the integers on both sides of
// it, ceil(cc) == ceil(cc').  The lane reports `safe`; otherwise the caller
// evaluates the exact expression (integer-aligned vertices hit that path,
// arbitrary geometry essentially never).
__device__ __forceinline__ f64 crossing_ceil(f64 b, f64 s, f64 c, bool& safe) {
    const f64 v = b * s;
    const f64 cc = v + c;
    const f64 k = ceil(cc);
    const f64 eps = (fabs(v) + fabs(cc)) * 0x1p-50 + 0x1p-1000;
    safe = safe && (cc - (k - 1.0) > eps) && (k - cc > eps);
    return k;
}

// row_span_in with the per-edge slopes (no division unless a crossing lies
// within eps of an integer, see crossing_ceil): the same [xs, xe).  (k_vis
// uses this form; row_span_in is its reference statement, and both are
// checked against row_span in tests/test_oracle.py.)
__device__ __forceinline__ void row_span_slopes(const f64 (&sx)[3], const f64 (&sy)[3], const f64 (&sl)[3], f64 y,
                                                f64 x0, f64 wlim, int& xs, int& xe) {
    const bool b0 = sy[0] > y, b1 = sy[1] > y, b2 = sy[2] > y;
    const bool v1 = (b1 != b0) && (b1 != b2);
    const bool v2 = (b2 != b0) && (b2 != b1);
    const f64 aix = v1 ? sx[2] : sx[0], aiy = v1 ? sy[2] : sy[0], sa = v1 ? sl[2] : sl[0];
    const f64 bix = v2 ? sx[2] : sx[1], biy = v2 ? sy[2] : sy[1], sb = v2 ? sl[2] : sl[1];
    bool safe = true;
    f64 ka = crossing_ceil(y - aiy, sa, aix, safe);
    f64 kb = crossing_ceil(y - biy, sb, bix, safe);
    if (!safe) {   // exact expression (cpp:832-839 order of operations)
        const f64 ajx = v1 ? sx[1] : sx[2], ajy = v1 ? sy[1] : sy[2];
        const f64 bjx = v2 ? sx[1] : sx[0], bjy = v2 ? sy[1] : sy[0];
        ka = ceil((ajx - aix) * (y - aiy) / (ajy - aiy) + aix);
        kb = ceil((bjx - bix) * (y - biy) / (bjy - biy) + bix);
    }
    xs = (int)clampd(fmin(ka, kb) - x0, 0.0, wlim);
    xe = (int)clampd(fmax(ka, kb) - x0, 0.0, wlim);
}

// ---- f32 fast path of row_span_slopes (k_vis) -----------------------------
// The two straddling edges of a row are the two edges at the vertex alone on
// its side of the row: the edges at the lowest-y vertex above the middle
// vertex's y (L = min-max, T = min-mid), at the highest-y vertex from there on
// (L, B = mid-max) -- row_span_in's selection, made once per triangle.  Each
// crossing cc = (y - yi) * s + xi is evaluated in f32 relative to the tile
// origin (xi - x0, yi - y0: exact in f64, small), which is cheap (f32 issues at
// twice the f64 rate) and whose error bound is small:
//   |cc32 - cc| <= 2^-24 (|cc| + 4|v| + |xr|) + |s| (|yr| 2^-48 + |yi| 2^-53)
//                  + |xi| 2^-53 + (the f64 expression's own rounding, 2^-50 (|v| + |cc|))
// (v = (y - yi) s; the bound used, eps = 2^-22 |cc32| + 2^-20 |v32| + ce, has a
// factor 4 of margin and ce per edge).  When cc32 is further than eps from the
// integers on both sides, ceil(cc32) is the exact expression's ceil; otherwise
// (or for non-finite / huge values: eps or cc32 not finite) the row takes
// row_span_slopes, which is itself exact.
struct Edge32 {
    float x, yhi, ylo, s, ce;   // anchor vertex relative to the tile origin (y as hi + lo), slope, error term
};

__device__ __forceinline__ Edge32 edge32(f64 xi, f64 yi, f64 s, f64 x0, f64 y0) {
    Edge32 e;
    const f64 xr = xi - x0, yr = yi - y0;
    e.x = (float)xr;
    e.yhi = (float)yr;
    e.ylo = (float)(yr - (f64)e.yhi);
    e.s = (float)s;
    const float as = fabsf(e.s);
    e.ce = fabsf(e.x) * 0x1p-21f + as * (fabsf(e.yhi) * 0x1p-46f + (float)(fabs(yi) * 0x1p-51)) +
           (float)(fabs(xi) * 0x1p-51) + 0x1p-23f;
    return e;
}

// Per-triangle edge selection: L (min-y vertex to max-y vertex), T (min-mid),
// B (mid-max), each as pointInPolygon's edge k anchored at vertex k (edge_slopes);
// ymid = the middle vertex's y (rows y < ymid use L and T, the others L and B).
struct Span32 {
    Edge32 L, T, B;
    f64 ymid;
};

__device__ __forceinline__ Span32 span32_setup(const f64 (&sx)[3], const f64 (&sy)[3], const f64 (&sl)[3], f64 x0,
                                               f64 y0) {
    const f64 a = sy[0], b = sy[1], c = sy[2];
    const int imin = (b < a) ? ((c < b) ? 2 : 1) : ((c < a) ? 2 : 0);
    const int imax = (b >= a) ? ((c >= b) ? 2 : 1) : ((c >= a) ? 2 : 0);
    const int imid = 3 - imin - imax;
    // edge id of vertex pair {p, q}: {0,2} -> 0, {0,1} -> 1, {1,2} -> 2 (sums 2, 1, 3)
    auto eid = [](int p, int q) { const int s = p + q; return s == 2 ? 0 : (s == 1 ? 1 : 2); };
    auto pick = [&](int k) {
        const f64 xi = k == 0 ? sx[0] : (k == 1 ? sx[1] : sx[2]);
        const f64 yi = k == 0 ? sy[0] : (k == 1 ? sy[1] : sy[2]);
        const f64 si = k == 0 ? sl[0] : (k == 1 ? sl[1] : sl[2]);
        return edge32(xi, yi, si, x0, y0);
    };
    Span32 S;
    S.L = pick(eid(imin, imax));
    S.T = pick(eid(imin, imid));
    S.B = pick(eid(imid, imax));
    S.ymid = imid == 0 ? a : (imid == 1 ? b : c);
    return S;
}

__device__ __forceinline__ float crossing32(const Edge32& e, float rf, bool& ok) {
    const float bb = (rf - e.yhi) - e.ylo;
    const float v = bb * e.s;
    const float cc = v + e.x;
    const float k = ceilf(cc);
    const float d = k - cc;   // in [0, 1), exact
    const float eps = fmaf(fabsf(cc), 0x1p-22f, fmaf(fabsf(v), 0x1p-20f, e.ce));
    ok = ok && (d > eps) && ((1.0f - d) > eps);
    return k;
}

// Row r of the tile (y = y0 + r, a row with exactly two straddling edges):
// the span [xs, xe) relative to x0, clamped to [0, wlim], when the f32 bound
// proves it (returns true); false: the caller evaluates row_span_slopes.
__device__ __forceinline__ bool row_span32(const Span32& S, int r, f64 y, float wlim, int& xs, int& xe) {
    const bool top = y < S.ymid;
    const Edge32& E = top ? S.T : S.B;
    const float rf = (float)r;
    bool ok = true;
    const float ka = crossing32(S.L, rf, ok);
    const float kb = crossing32(E, rf, ok);
    const float lo = fminf(ka, kb), hi = fmaxf(ka, kb);
    xs = (int)fminf(fmaxf(lo, 0.0f), wlim);
    xe = (int)fminf(fmaxf(hi, 0.0f), wlim);
    return ok;
}

// The key cache's capture table, in device memory (nr_free_vis.hip, capture_keys): the address of the slots (TH * TW
// keys each) and every tile's slot, ~0 for a tile that is not cached (no kept pair, or another rank's).
struct KeyCaptureTable {
    u64* keys;
    u32 slot[2];   // (one per tile: the table is allocated to the frame's tiles)
};

// State snapshot of one draw call (passed by value to the kernels).  The rasters' kernels take it in front of their
// other arguments, so its size, 304 bytes, is part of every instance's kernarg layout: a new field must fit into
// padding (or replace a field) and leave sizeof and every existing offset as they are -- the static_assert below
// the struct guards the size.  Every copy of a snapshot is a struct copy.
struct FrameParams {
    TriSrc src;
    f64 m[6];
    f64 ct[4];
    f64* fb;
    u32* depth;
    i64 W, H;
    int ipp;
    int tiles_x, tiles_y;
    int period;   // owned tile rows (BinParams)
    u64 mask;
    int depthTest, depthWrite;
    int pendColor;
    int wrapU;    // textured batches: the wrap state of the columns (TexWrap::u; 0: clamp) -- in what was padding
    f64 pendColorValue;
    int pendDepth;
    u32 pendDepthValue;
    unsigned long long* fragCounter;   // non-null: count covered fragments
    iu8* frameU8;                      // non-null: resolve also writes the frame output: the u8
                                       // image (cpp:52-57), or with frameYUV its YUV420P planes
    int frameYUV;
    int wrapV;        // ... and of the rows (TexWrap::v), likewise
    u32* tileStamp;   // non-null: k_vis leaves an empty tile's pending clears pending (stamps it tileEpoch,
    u32 tileEpoch;    // RenderContext::tileStamp) and writes only its frame output
    u64* tstamp;      // non-null (kernel timing): {~first start, last end} of the raster on the device's
                      // 100 MHz clock (raster_stamp_begin / _end, nr_timing_stamp)
    TexView tex;      // textured batches: the texture (a snapshot when it aliases fb)
    union {           // (one place in the snapshot: a batch is never both, and the other instances read neither)
        u32* winMask;                  // a marking frame (k_vis MARK instances only): bit t is set when triangle t wins a pixel
        const KeyCaptureTable* kcap;   // the key cache's capture frame (k_vis KCAP instances only): where its keys go
    };
    // perspective batches (attr_persp): each corner's 1/w, n*3 laid out like src.z (else null).  Only the shading reads it,
    // so it lives here and not in TriSrc, and last: the binning's BinParams and every offset of the snapshot
    // the existing instances read stay as they were.
    const f64* q;
    __host__ __device__ TexWrap wrap() const { return TexWrap{wrapU, wrapV}; }
};
// (the wrap state sits in the snapshot's padding: the kernels take the snapshot by value in front of their other
// arguments, so a snapshot of another size would move those arguments for every instance)
static_assert(sizeof(FrameParams) == 304, "the snapshot's size is part of every raster kernel's argument layout");

// Texel of a fragment's interpolated (u, v), as an offset in doubles: the
// texel the reference sampler picks (cpp:555-573: x < 0 -> 0, x >= w-1 ->
// w-2, then y the same way, texel ((i64)y, (i64)x)).  Its two clamps and the
// truncation are one max and one min here: for x < 0 both give 0; for 0 <= x <
// w-2 neither changes x; for w-2 <= x < w-1 the reference keeps x, which
// truncates to w-2 = min(x, w-2); for x >= w-1 both give w-2.  A NaN
// coordinate is undefined in the reference ((i64)NaN) and defined here as
// coordinate 0: fmax(NaN, 0) is 0.  With w, h >= 2 the offset
// is in range for every input: column in [0, w-2], row in [0, h-2].
__device__ __forceinline__ i64 tex_index(const TexView& tv, f64 x, f64 y) {
    const int xi = (int)fmin(fmax(x, 0.0), tv.xlast);
    const int yi = (int)fmin(fmax(y, 0.0), tv.ylast);
    return (i64)yi * tv.pitch + xi * tv.ipp;
}

// The bilinear filter's footprint of a fragment's (u, v) (the
// filter in the reference sampler's body, cpp:576-619): the offset of texel
// (iy, ix) -- its neighbours are tv.ipp and tv.pitch doubles further -- and the
// fractions fu, fv.  The reference clamps x < 0 -> 0, x >= w-1 -> w-2 (so the
// +1 neighbour exists), then ix = (i64)x, fu = x - ix.  That needs w-1, which
// as xlast + 1.0 is one more loop-invariant vector value (see TexView); the
// form here needs xlast and the constant 1 only: x' = fmax(x, 0) (NaN -> 0),
// ix = (int)fmin(x', xlast), fu = x' - ix, and fu >= 1 -> 0.  For x' < w-2 both
// forms truncate x' itself; for w-2 <= x' < w-1 the reference keeps x', ix is
// w-2 and x' - (w-2) is exact and below 1; for x' >= w-1 (or +inf) the
// difference is >= 1 or infinite and becomes the reference's 0.  Rows likewise.
// All four texels are in range for every input: ix <= w-2, iy <= h-2.
// (tests/test_bilinear_ref.py proves the two forms equal.)
__device__ __forceinline__ i64 tex_bilinear(const TexView& tv, f64 x, f64 y, f64& fu, f64& fv) {
    const f64 xc = fmax(x, 0.0), yc = fmax(y, 0.0);
    const int xi = (int)fmin(xc, tv.xlast);
    const int yi = (int)fmin(yc, tv.ylast);
    const f64 du = xc - (f64)xi, dv = yc - (f64)yi;
    fu = du < 1.0 ? du : 0.0;
    fv = dv < 1.0 ? dv : 0.0;
    return (i64)yi * tv.pitch + xi * tv.ipp;
}
// One channel of the filtered colour from its four texels c0 (iy, ix), c1 (iy, ix+1), c2 (iy+1, ix), c3 (iy+1,
// ix+1), as C evaluates cpp:609: each product left to right, the sum left to right, every operation rounded (the
// build has no FMA contraction).  gu = 1 - fu, gv = 1 - fv.
__device__ __forceinline__ f64 bilinear_mix(f64 c0, f64 c1, f64 c2, f64 c3, f64 fu, f64 fv, f64 gu, f64 gv) {
    return c0 * gu * gv + c1 * fu * gv + c2 * gu * fv + c3 * fu * fv;
}

// (f64)p of an integer 2 <= p < 2^30 by integer operations -- exponent from the leading bit, the rest shifted into
// the mantissa, exact -- so that the period of a batch's fold, uniform over the batch, is formed in scalar registers.
__device__ __forceinline__ f64 wrap_period(int p) {
    const int e = 31 - __builtin_clz((u32)p);
    const u64 bits = ((u64)(1023 + e) << 52) | (((u64)(u32)p << (52 - e)) & 0x000FFFFFFFFFFFFFull);
    return __longlong_as_double((long long)bits);
}
// One axis of a footprint under the batch's wrap state (DESIGN.md §3 "Wrap addressing"; the rule for columns with n =
// w, x = u and for rows with n = h, x = v): the texel index c0, the signed step d to the bilinear +1 neighbour (c1 -
// c0) and the fraction f.  Mode 0 is tex_index's / tex_bilinear's axis: (i, +1, f).  Otherwise, with P = (f64)n
// (repeat) or (f64)(2n) (mirror), in f64, every operation rounded in the order written (no contraction in this
// build), the divide IEEE:
//   k = floor(x / P);  t = x - k * P;  !(t >= 0) -> 0 (NaN, inf - inf, a t rounding left negative);  t >= P -> 0 (a t
//   rounding left at P, the garbage of a huge |x|);  i0 = (int)t in 0 .. P-1, f = t - i0 (exact, in [0, 1));  i1 = i0 +
//   1, P -> 0;  c(j) = j (repeat), j < n ? j : 2n - 1 - j (mirror).
// Every input gives indices in [0, n-1].  The step is +1, 0 (a mirror seam: the same texel twice), -1 (the mirror's
// descending half) or -(n-1) (the repeat seam): a footprint is its base texel and two signed strides, not four offsets.
// (ax: one axis of the state, mode | n << 2; last: the clamp axis's bound, TexView::xlast / ylast.  On a clamped
// axis a -0.0 coordinate counts as 0 and its fraction is a zero of either sign, as in tex_bilinear: fmax(-0.0, 0.0)
// may return either zero; tests/test_wrap_ref.py leaves that one value out of the mode-0 comparison of the forms.)
__device__ __forceinline__ void wrap_fold(f64 x, int ax, f64 last, int& c0, int& d, f64& f) {
    const int mode = ax & 3, n = ax >> 2;
    if (mode == 0) {
        const f64 xc = fmax(x, 0.0);
        c0 = (int)fmin(xc, last);
        const f64 dd = xc - (f64)c0;
        f = dd < 1.0 ? dd : 0.0;
        d = 1;
        return;
    }
    const int per = mode == 2 ? 2 * n : n;
    const f64 P = wrap_period(per);
    const f64 k = floor(x / P);
    f64 t = x - k * P;
    if (!(t >= 0.0)) t = 0.0;
    if (t >= P) t = 0.0;
    const int i0 = (int)t;
    f = t - (f64)i0;
    int i1 = i0 + 1;
    if (i1 == per) i1 = 0;
    if (mode == 2) {
        c0 = i0 < n ? i0 : per - 1 - i0;
        d = (i1 < n ? i1 : per - 1 - i1) - c0;
    } else {
        c0 = i0;
        d = i1 - i0;
    }
}
// tex_index under a wrap state: the row term of the offset is 64-bit, as there.  (The step and the fraction
// wrap_fold also returns are not used here: nothing reads them, and the compiler drops their computation.)
__device__ __forceinline__ i64 tex_index_wrap(const TexView& tv, const TexWrap& tw, f64 x, f64 y) {
    int xi, yi, d;
    f64 f;
    wrap_fold(x, tw.u, tv.xlast, xi, d, f);
    wrap_fold(y, tw.v, tv.ylast, yi, d, f);
    return (i64)yi * tv.pitch + xi * tv.ipp;
}
// tex_bilinear under a wrap state: the offset of texel (r(j0), c(i0)) and the steps, in texels, to the +1 column and
// the +1 row (the clamp path's are +1 and +1: tv.ipp and tv.pitch doubles).  A caller scales them itself (tex_quad_strides): kept
// in texels they are two ints across a gather; the row stride in doubles can exceed 32 bits for a tall texture.
__device__ __forceinline__ i64 tex_bilinear_wrap(const TexView& tv, const TexWrap& tw, f64 x, f64 y, f64& fu, f64& fv,
                                                 int& du, int& dv) {
    int xi, yi;
    wrap_fold(x, tw.u, tv.xlast, xi, du, fu);
    wrap_fold(y, tw.v, tv.ylast, yi, dv, fv);
    return (i64)yi * tv.pitch + xi * tv.ipp;
}
__device__ __forceinline__ void tex_quad_strides(const TexView& tv, int du, int dv, i64& dcol, i64& drow) {
    dcol = du * tv.ipp;
    drow = (i64)dv * tv.pitch;
}

// Kernel timing of the rasters by the device's constant 100 MHz clock
// (s_memrealtime): the first workgroups dispatched on each XCD (blockIdx < 8)
// max-in the inverted start time, every workgroup the end time -- the
// kernel's execution span, as rocprofv3's kernel trace measures it, with no
// packet on the stream (events around or bound to the launch add the launch
// gap to the time; profiles/r06/ab_event_every.txt).
__device__ __forceinline__ void raster_stamp_begin(const FrameParams& fp) {
    if (fp.tstamp && threadIdx.x == 0 && blockIdx.x < 8)
        atomicMax(reinterpret_cast<unsigned long long*>(&fp.tstamp[0]), ~__builtin_amdgcn_s_memrealtime());
}
__device__ __forceinline__ void raster_stamp_end(const FrameParams& fp) {
    if (fp.tstamp && threadIdx.x == 0)
        atomicMax(reinterpret_cast<unsigned long long*>(&fp.tstamp[1]), __builtin_amdgcn_s_memrealtime());
}

// Frame output of pixel p = (px, py) from its framebuffer value, written by
// the rasters' own write-back when they cover every owned pixel (a pending
// clear): the u8 image (cpp:52-57) or, with fp.frameYUV, its YUV420P planes --
// Y of every pixel, U and V from the even pixel of each 2x2 block (tiles have
// even sizes and origins, so a block never straddles two).
// Output stores of the rasters' shading passes (framebuffer, depth, frame
// output): written once per frame and not read again by the kernel, so
// non-temporal (streaming) stores -- round 6, with the fast clear and the
// binning beside the raster: C3 -2.5 %, an 8-way share -2.6 %, 1080p and C2
// within 1 % (profiles/r06/ab_ntst.txt; round 3, frame outputs only: +-2 %).
template <class T>
__device__ __forceinline__ void out_store(T* p, T v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_frame_out(const FrameParams& fp, i64 p, i64 px, i64 py, f64 cr, f64 cg, f64 cb,
                                                f64 ca) {
    if (!fp.frameU8) return;
    const int r8 = nr_to_u8(cr), g8 = nr_to_u8(cg), b8 = nr_to_u8(cb);
    if (fp.frameYUV) {
        out_store<iu8>(fp.frameU8 + p, (iu8)nr_y_of(r8, g8, b8));
        if (!((px | py) & 1)) {
            const i64 cw = fp.W >> 1;
            iu8* up = fp.frameU8 + fp.W * fp.H + (py >> 1) * cw + (px >> 1);
            out_store<iu8>(up, (iu8)nr_u_of(r8, g8, b8));
            out_store<iu8>(up + cw * (fp.H >> 1), (iu8)nr_v_of(r8, g8, b8));
        }
    } else {
        iu8* d8 = fp.frameU8 + p * fp.ipp;
        out_store<iu8>(d8, (iu8)r8); out_store<iu8>(d8 + 1, (iu8)g8); out_store<iu8>(d8 + 2, (iu8)b8);
        if (fp.ipp == 4) out_store<iu8>(d8 + 3, (iu8)nr_to_u8(ca));
    }
}

// Per-triangle setup record of the ordered raster, formed once per triangle
// by the counting kernel (k_tri_count, or k_free_count for a binned ordered batch) (a triangle of C5 lies in ~100 tiles; the raster used to set
// it up again in each): screen vertices, edge slopes, 1/den, depths and the
// depth-pass bound (zpass_bound).  16 doubles, 128 B, 16-B aligned.
enum { R_X0 = 0, R_Y0, R_X1, R_Y1, R_X2, R_Y2, R_SL0, R_SL1, R_SL2, R_INV, R_Z0, R_Z1, R_Z2, R_FLAGS, ORec = 16 };

// Depth-pass proof (zpass_all): with the Z test on and Z write off, a
// triangle passes the LESS test on every pixel the exact span rule covers when
// all of them quantise (nr_quantize_depth) strictly below the tile's smallest
// depth zmin.  For a triangle with G = max|edge| / |den|, bbox extent S and
// coordinate magnitude M, G*S <= 1e4 and G*M <= 1e4 bound the computed
// barycentrics of covered pixels to [-1e-10, 1 + 1e-10] (span-rule crossings
// and the w1/w2 expressions both err by O(u (G S + G M)), u = 2^-53; den's
// cancellation by O(u G S) relative), so with |z| <= 2 the computed depth is at
// most max(z) + 1e-9 (< max(z) + 1e-8, the bound used).  The triangle-only
// part is this bound, quantised, or 0xFFFFFFFF when the analysis does not
// apply (no tile minimum lies above it): zpass_all == (zpass_bound < zmin).
__device__ __forceinline__ u32 zpass_bound(const f64 (&sx)[3], const f64 (&sy)[3], f64 e1x, f64 e1y, f64 e2x, f64 e2y,
                                           f64 den, f64 z0, f64 z1, f64 z2) {
    if (!tri_finite(sx, sy) || den == 0) return 0xFFFFFFFFu;
    if (!(fabs(z0) <= 2 && fabs(z1) <= 2 && fabs(z2) <= 2)) return 0xFFFFFFFFu;   // (NaN: no bound)
    const f64 xmn = fmin(fmin(sx[0], sx[1]), sx[2]), xmx = fmax(fmax(sx[0], sx[1]), sx[2]);
    const f64 ymn = fmin(fmin(sy[0], sy[1]), sy[2]), ymx = fmax(fmax(sy[0], sy[1]), sy[2]);
    const f64 e = fmax(fmax(fabs(e1x), fabs(e1y)), fmax(fabs(e2x), fabs(e2y)));
    const f64 G = e / fabs(den);
    const f64 S = (xmx - xmn) + (ymx - ymn) + 4.0;
    const f64 M = fmax(fmax(fabs(xmn), fabs(xmx)), fmax(fabs(ymn), fabs(ymx))) + 1.0;
    if (!(G * S <= 1e4 && G * M <= 1e4)) return 0xFFFFFFFFu;
    return nr_quantize_depth(fmax(fmax(z0, z1), z2) + 1e-8);
}

// Setup record of triangle t (screen vertices sx, sy, valid: finite, den != 0).
__device__ __forceinline__ void write_ordered_record(f64* rec, i64 t, const f64 (&sx)[3], const f64 (&sy)[3],
                                                     const f64* zsrc) {
    const f64 e1x = sx[1] - sx[0], e1y = sy[1] - sy[0], e2x = sx[2] - sx[0], e2y = sy[2] - sy[0];
    const f64 den = e1x * e2y - e2x * e1y;
    f64 sl[3];
    edge_slopes(sx, sy, sl);
    f64 z0 = 0, z1 = 0, z2 = 0;
    if (zsrc) { z0 = zsrc[t * 3]; z1 = zsrc[t * 3 + 1]; z2 = zsrc[t * 3 + 2]; }
    const u64 flags = 1ull | ((u64)zpass_bound(sx, sy, e1x, e1y, e2x, e2y, den, z0, z1, z2) << 32);
    double2* r = reinterpret_cast<double2*>(rec + t * ORec);
    r[0] = make_double2(sx[0], sy[0]);
    r[1] = make_double2(sx[1], sy[1]);
    r[2] = make_double2(sx[2], sy[2]);
    r[3] = make_double2(sl[0], sl[1]);
    r[4] = make_double2(sl[2], 1.0 / den);
    r[5] = make_double2(z0, z1);
    r[6] = make_double2(z2, __longlong_as_double((long long)flags));
}

enum Opacity { OPQ_UNKNOWN = 0, OPQ_OPAQUE, OPQ_BLENDED };

// Words of a binned batch's plan (k_free_plan*): the device copy (a set's
// dplan, the schedule's, a gate's gplan) holds the first PW_DEV, read by the
// kernels after the plan; the host copy (FreeSet::hplan) all PW_COUNT.
enum PlanWord {
    PW_PAIRS = 0,   // (tile, triangle) pairs
    PW_ITEMS,       // k_vis work items
    PW_SPLIT,       // slices of split tiles
    PW_FITS,        // the list, items and key slots had room (ordered: and every list fits the LDS sort)
    PW_DEV,
    PW_SEQ = PW_DEV,   // the batch's sequence number
    PW_HEAVY,          // dense tiles
    PW_LONGEST,        // longest tile list (ordered batches; else 0)
    PW_COUNT
};

bool grow_temp(TriScratch& sc, size_t need);

// Pointers to a triangle soup, on the host or the device: xy n*6, z n*3 or null, the attribute array (colours or
// uv, by the batch's mode), q n*3 (a perspective textured soup's 1/w per corner) or null.
struct Soup {
    const f64* xy;
    const f64* z;
    const f64* attr;
    const f64* q;
    i64 n;
};

// What one triangle draw hands to the rasters: the host-side description of a batch, built on the caller's
// stack and passed by reference down to the snapshot (frame_params).
// callerOwned is true exactly when some array the batch reads (xy, z, the attributes, q) is still the caller's
// device memory.  Such a batch is sized exactly inside the call (a host wait for its binning) and never re-run
// later: after the call returns nothing of the library may read the caller's arrays again.  Arrays of the
// context's staging, of a TriangleBuffer or of a mesh draw are not the caller's.
struct Batch {
    TriSrc src;
    const f64* q;                                 // perspective textured batches: the corners' 1/w (else null)
    bool modulated = false;                       // textured: src.attr is n*18, uv and colour per corner (q is set)
    TexView tex = tex_view(nullptr, 2, 2, false); // textured modes: what draw_textured resolved
    TexWrap wrap = TexWrap{0, 0};                 // textured modes: the context's wrap state when the draw was issued
    Opacity opq;
    TriangleBuffer* tb;   // non-null: the batch is that (immutable) buffer -- its binning may overlap the previous
                          // raster, and a repeat draw is sized from its known totals
    bool callerOwned;
};
inline Batch soup_batch(const Soup& s, int mode, Opacity opq, TriangleBuffer* tb, bool callerOwned) {
    Batch b;
    b.src = TriSrc{s.xy, s.z, s.attr, mode, s.n};
    b.q = s.q;
    b.opq = opq;
    b.tb = tb;
    b.callerOwned = callerOwned;
    return b;
}

FrameParams frame_params(RenderContext* ctx, const Batch& b);
inline BinParams bin_params(const FrameParams& fp) {   // the binning's view of the same snapshot
    BinParams bp;
    bp.src = fp.src;
    for (int k = 0; k < 6; ++k) bp.m[k] = fp.m[k];
    bp.W = fp.W; bp.H = fp.H; bp.tiles_x = fp.tiles_x;
    bp.period = fp.period; bp.mask = fp.mask;
    set_owned_rows(bp, fp.tiles_y);
    return bp;
}
void finish_batch(RenderContext* ctx, const FrameParams& fp);
u32* tile_stamps(RenderContext* ctx, i64 ntiles);   // the context's tile stamps, next epoch (nr_tri.hip)

// the two rasterisers (host side)
// ordered batches: binned like the order-free ones (count / plan / emit, on the
// binning stream beside the previous raster) when the frame has at most
// ORD_BIN_TILES tiles, each tile's list sorted in LDS (k_tile_sort); the
// global-sort path (draw_ordered_sorted) otherwise, and for a batch with a tile
// of more than ORD_SORT_CAP triangles (detected by the plan, re-run)
void draw_ordered(RenderContext* ctx, const Batch& b);
// (fp.src == bp.src is the batch)
void draw_ordered_sorted(RenderContext* ctx, const FrameParams& fp, const BinParams& bp);
// the same kernels for a deferred re-run (nr_settle): the batch's snapshot only, context flags untouched
void rerun_ordered_sorted(RenderContext* ctx, const FrameParams& fp, const BinParams& bp);
constexpr u32 ORD_SORT_CAP = 8192;    // longest tile list the ordered raster sorts in LDS
constexpr int ORD_BIN_TILES = 16384;  // tiles of the binned ordered path (the register plan kernel's limit)
// binned ordered batches: k_tile_sort sorts each tile's list [off[t], off[t + 1])
// in place (binning stream), then the raster runs one workgroup per tile; both
// are no-ops unless plan[PW_FITS]
void launch_tile_sort(const u32* off, u32* list, const u32* plan, int ntiles, hipStream_t s, hipEvent_t stop);
void launch_ordered_binned(const FrameParams& fp, const u32* list, const u32* off, const u32* plan, const f64* rec,
                           int ntiles, hipStream_t s, hipEvent_t start, hipEvent_t stop);
// b.tb and b.callerOwned: see Batch
void draw_free(RenderContext* ctx, const Batch& b, bool ordered);
void settle(RenderContext* ctx);
i64 visible_pairs(RenderContext* ctx);   // pairs kept in the schedule's visible list (0: none)
bool visible_plan_totals(RenderContext* ctx, i64* out4);   // the visible plan's pairs, items, split slices, dense tiles
bool key_cache_totals(RenderContext* ctx, i64* out3);      // the key cache's cached tiles, key items, bytes of keys
bool key_record_totals(RenderContext* ctx, i64* out3);     // the key records' slots, records, bytes
bool key_index_totals(RenderContext* ctx, i64* out4);      // the key index's tiles, staged winners, direct pixels, bytes

// the batch entry points behind every triangle draw call (nr_tri.hip), shared with the mesh front end
// (nr_mesh.hip): draw picks the raster; draw_textured first completes the batch from the texture (its view, the
// mode by b.q and b.modulated, the opacity by the texture's alpha and, modulated, the corner alphas).  check_texture: a texture's preconditions, an error latched
// under the caller's name `what` when one fails
void draw(RenderContext* ctx, const Batch& b);
bool check_texture(RenderContext* ctx, const Texture* tex, const char* what);
void draw_textured(RenderContext* ctx, Texture* tex, Batch& b);

}  // namespace nrtri
