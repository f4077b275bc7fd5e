// nr_morph.hip — morph targets (blend shapes) on the device, alone or fused with
// linear-blend skinning (DESIGN.md §3 "Morph targets").
//
// A MeshMorph keeps, for nv vertices and T targets, base positions and T position
// deltas, and either both or neither of base normals and T normal deltas.  A call
// hands over T weights and ONE kernel rewrites the mesh's positions (and, for a lit
// mesh under a morph with normals, its normals); every draw issued afterwards
// reads them through the kernels it has always run.
//
// Per vertex and component, f64, every product and sum rounded in the order
// written (the build has no FMA contraction), no division, no renormalisation:
//   X = px;  for t = 0 .. T-1 in index order:  if w_t == 0.0 skip;  X = X + w_t * dPx[t][v]
// The skip is part of the definition: a target under a zero weight (either sign)
// contributes nothing, whatever its deltas hold; a NaN weight is not zero.
// PoseMeshMorphed forms (X, Y, Z) and (NX, NY, NZ) in registers and feeds them to
// skinning's expressions in place of the skin's bind pose.
//
// Layout: the arrays are target-major, each target's nv*3 doubles padded to an
// even count (`stride`), so that the morph-only kernel is a flat pass of 16-byte
// loads over base and deltas and a wave reads one contiguous run per active target.
// The weights are the same in every lane: the first wave of a block compacts the
// non-zero ones, in index order, into a list in LDS, and the loop over that list
// issues the loads of MORPH_UNROLL targets before their dependent sums.  A
// zero-weight target is never loaded.
//
// Ordering is PoseMesh's (nr_skin.hip): the kernel runs on the context's stream,
// between the draws issued before and after the call; host weights (and, fused,
// the palette) travel through ONE of the context's pinned buffers into the
// morph's (and the skin's) own device copies by asynchronous copies on that stream.
#include "nr_mesh.h"

#include <cstdint>
#include <cstring>

struct MeshMorph {
    i64 nv = 0, T = 0;
    int device = 0;
    i64 stride = 0;            // doubles per target: nv*3 rounded up to even
    f64* pos = nullptr;        // base positions, `stride` doubles (the padding is zero)
    f64* normal = nullptr;     // base normals, or null
    f64* dpos = nullptr;       // T * stride
    f64* dnormal = nullptr;    // T * stride, or null
    f64* weights = nullptr;    // T: where host weights land
};

namespace {

constexpr int MORPH_MAX_TARGETS = 1024;
constexpr int MORPH_UNROLL = 4;   // targets whose loads are in flight before the first dependent sum

// The active targets of a call: (t, w_t) for every w_t that is not zero, in index order.
struct ActiveList {
    u32 t[MORPH_MAX_TARGETS];
    f64 w[MORPH_MAX_TARGETS];
    u32 n;
};

// Built by the block's first wave, 64 weights a round (T <= MORPH_MAX_TARGETS: checked at creation), then the
// barrier: every thread of the block calls it.  NaN != 0.0, so a NaN weight is listed.
__device__ __forceinline__ void build_active_list(ActiveList& L, const f64* __restrict__ w, u32 T) {
    if (threadIdx.x < 64u) {
        u32 n = 0;
        for (u32 t0 = 0; t0 < T; t0 += 64u) {
            const u32 t = t0 + threadIdx.x;
            const f64 wt = t < T ? w[t] : 0.0;
            const bool on = wt != 0.0;
            const unsigned long long mask = __ballot(on);
            if (on) {
                const u32 k = n + (u32)__popcll(mask & ((1ull << threadIdx.x) - 1ull));
                L.t[k] = t;
                L.w[k] = wt;
            }
            n += (u32)__popcll(mask);
        }
        if (threadIdx.x == 0) L.n = n;
    }
    __syncthreads();
}

// acc = acc + w_t * load(t) over the active targets in index order; `load(t)` fetches this thread's deltas of
// target t and `add(acc, d, w)` is the rounded product and sum per component.  Only the loads are hoisted.
template <class Acc, class Load, class Add>
__device__ __forceinline__ void for_active_targets(const ActiveList& L, Acc& acc, Load load, Add add) {
    const u32 n = L.n;
    u32 k = 0;
    for (; k + MORPH_UNROLL <= n; k += MORPH_UNROLL) {
        decltype(load(0u)) d[MORPH_UNROLL];
#pragma unroll
        for (int u = 0; u < MORPH_UNROLL; ++u) d[u] = load((u32)__builtin_amdgcn_readfirstlane((int)L.t[k + u]));
#pragma unroll
        for (int u = 0; u < MORPH_UNROLL; ++u) add(acc, d[u], L.w[k + u]);
    }
    for (; k < n; ++k) add(acc, load((u32)__builtin_amdgcn_readfirstlane((int)L.t[k])), L.w[k]);
}

template <bool NRM>
struct Pair2 { double2 p, n; };   // two consecutive doubles of the flat position (and normal) array

// MorphMesh: a flat pass, one thread per two doubles of the nv*3: 16 B of base and 16 B per active target in, 16 B
// out; NRM: the same for the normals.  `n3` = nv*3 (the last thread of an odd n3 stores one double), `stride2` =
// the target stride in double2.
template <bool NRM>
__global__ __launch_bounds__(256) void k_mesh_morph(const double2* __restrict__ bpos, const double2* __restrict__ bnrm,
                                                    const double2* __restrict__ dpos, const double2* __restrict__ dnrm,
                                                    i64 stride2, const f64* __restrict__ weights, u32 T, i64 n3,
                                                    f64* __restrict__ pos, f64* __restrict__ nrm) {
    __shared__ ActiveList L;
    build_active_list(L, weights, T);
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= stride2) return;
    Pair2<NRM> a;
    a.p = bpos[i];
    if constexpr (NRM) a.n = bnrm[i];
    for_active_targets(
        L, a,
        [&](u32 t) {
            Pair2<NRM> d;
            d.p = dpos[(i64)t * stride2 + i];
            if constexpr (NRM) d.n = dnrm[(i64)t * stride2 + i];
            return d;
        },
        [](Pair2<NRM>& acc, const Pair2<NRM>& d, f64 w) {
            acc.p.x = acc.p.x + w * d.p.x;
            acc.p.y = acc.p.y + w * d.p.y;
            if constexpr (NRM) {
                acc.n.x = acc.n.x + w * d.n.x;
                acc.n.y = acc.n.y + w * d.n.y;
            }
        });
    if (2 * i + 1 < n3) {
        *reinterpret_cast<double2*>(pos + 2 * i) = a.p;
        if constexpr (NRM) *reinterpret_cast<double2*>(nrm + 2 * i) = a.n;
    } else {   // (the padding of an odd nv*3 is computed and dropped)
        pos[2 * i] = a.p.x;
        if constexpr (NRM) nrm[2 * i] = a.n.x;
    }
}

template <bool NRM>
struct Vert { f64 p[3], n[3]; };

// PoseMeshMorphed: one thread per vertex, as k_mesh_skin, whose bind position (and normal) is the morph's result,
// kept in registers; the skin contributes joints, weights and the palette (LDS: staged as k_mesh_skin stages it).
template <bool NRM, bool LDS>
__global__ __launch_bounds__(256) void k_mesh_morph_skin(const f64* __restrict__ bpos, const f64* __restrict__ bnrm,
                                                         const f64* __restrict__ dpos, const f64* __restrict__ dnrm,
                                                         i64 stride, const f64* __restrict__ mweights, u32 T,
                                                         const uint4* __restrict__ joints,
                                                         const double2* __restrict__ weights,
                                                         const double2* __restrict__ palette, u32 nb, i64 nv,
                                                         f64* __restrict__ pos, f64* __restrict__ nrm) {
    __shared__ ActiveList L;
    __shared__ f64 sh[LDS ? SKIN_LDS_MAX_BONES * SKIN_LDS_STRIDE : 1];
    if constexpr (LDS) {
        for (u32 i = threadIdx.x; i < nb * 6u; i += 256u) {   // (nb <= SKIN_LDS_MAX_BONES: checked by the launch)
            const double2 q = palette[i];
            const u32 b = i / 6u, e = i - b * 6u;
            sh[b * (u32)SKIN_LDS_STRIDE + 2u * e] = q.x;
            sh[b * (u32)SKIN_LDS_STRIDE + 2u * e + 1u] = q.y;
        }
    }
    build_active_list(L, mweights, T);   // (its barrier also covers the palette)
    const i64 v = (i64)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const uint4 j4 = joints[v];
    const double2 wa = weights[v * 2], wb = weights[v * 2 + 1];
    const u32 j[4] = {j4.x, j4.y, j4.z, j4.w};
    const f64 w[4] = {wa.x, wa.y, wb.x, wb.y};
    Vert<NRM> a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.p[c] = bpos[v * 3 + c];
        a.n[c] = NRM ? bnrm[v * 3 + c] : 0.0;
    }
    for_active_targets(
        L, a,
        [&](u32 t) {
            Vert<NRM> d;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d.p[c] = dpos[(i64)t * stride + v * 3 + c];
                d.n[c] = NRM ? dnrm[(i64)t * stride + v * 3 + c] : 0.0;
            }
            return d;
        },
        [](Vert<NRM>& acc, const Vert<NRM>& d, f64 wt) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc.p[c] = acc.p[c] + wt * d.p[c];
                if constexpr (NRM) acc.n[c] = acc.n[c] + wt * d.n[c];
            }
        });
    const f64 px = a.p[0], py = a.p[1], pz = a.p[2], nx = a.n[0], ny = a.n[1], nz = a.n[2];
    // from here on k_mesh_skin's expressions, term for term (DESIGN.md §3 "Skinned meshes")
    f64 X = 0, Y = 0, Z = 0, NX = 0, NY = 0, NZ = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Bone B = LDS ? load_bone_lds(sh, j[k]) : load_bone(palette, j[k]);
        const f64 xk = ((B.m[0] * px + B.m[1] * py) + B.m[2] * pz) + B.m[3];
        const f64 yk = ((B.m[4] * px + B.m[5] * py) + B.m[6] * pz) + B.m[7];
        const f64 zk = ((B.m[8] * px + B.m[9] * py) + B.m[10] * pz) + B.m[11];
        X = k == 0 ? w[k] * xk : X + w[k] * xk;
        Y = k == 0 ? w[k] * yk : Y + w[k] * yk;
        Z = k == 0 ? w[k] * zk : Z + w[k] * zk;
        if constexpr (NRM) {
            const f64 ak = (B.m[0] * nx + B.m[1] * ny) + B.m[2] * nz;
            const f64 bk = (B.m[4] * nx + B.m[5] * ny) + B.m[6] * nz;
            const f64 ck = (B.m[8] * nx + B.m[9] * ny) + B.m[10] * nz;
            NX = k == 0 ? w[k] * ak : NX + w[k] * ak;
            NY = k == 0 ? w[k] * bk : NY + w[k] * bk;
            NZ = k == 0 ? w[k] * ck : NZ + w[k] * ck;
        }
    }
    pos[v * 3] = X;
    pos[v * 3 + 1] = Y;
    pos[v * 3 + 2] = Z;
    if constexpr (NRM) {
        nrm[v * 3] = NX;
        nrm[v * 3 + 1] = NY;
        nrm[v * 3 + 2] = NZ;
    }
}

void free_morph(MeshMorph* mo) {
    for (void* p : {(void*)mo->pos, (void*)mo->normal, (void*)mo->dpos, (void*)mo->dnormal, (void*)mo->weights})
        if (p) NR_CHECK(hipFree(p));
    delete mo;
}

// `rows` host rows of n3 doubles into device rows of `stride` doubles (stride - n3 is 0 or 1).
void upload_rows(f64* dst, const f64* src, i64 rows, i64 n3, i64 stride, hipStream_t st) {
    NR_CHECK(hipMemcpy2DAsync(dst, (size_t)stride * sizeof(f64), src, (size_t)n3 * sizeof(f64), (size_t)n3 * sizeof(f64),
                              (size_t)rows, hipMemcpyHostToDevice, st));
}

// The four entry points under the caller's name: every check, then (host arrays) their hand-off through ONE
// pinned buffer, then the one kernel, on the context's stream.  `s` null: MorphMesh; else the fused call.
bool morph(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette, MeshMorph* mo, const f64* weights,
           bool fused, bool onDevice, const char* what) {
    if (!ctx) return fail(what, "NULL context");
    if (!m) return fail(what, "NULL mesh");
    if (fused && !s) return fail(what, "NULL skin");
    if (fused && !palette) return fail(what, "NULL palette");
    if (!mo) return fail(what, "NULL morph");
    if (!weights) return fail(what, "NULL weights");
    if (m->nv != mo->nv) return fail(what, "the mesh and the morph differ in their vertex count");
    if (fused && m->nv != s->nv) return fail(what, "the mesh and the skin differ in their vertex count");
    if (m->device != ctx->device || mo->device != ctx->device || (fused && s->device != ctx->device))
        return fail(what, fused ? "mesh, skin, morph and context are not on one device"
                                : "mesh, morph and context are not on one device");
    if (onDevice && (reinterpret_cast<uintptr_t>(weights) & 15u) != 0)
        return fail(what, "device weights must be 16-byte aligned");
    if (onDevice && fused && (reinterpret_cast<uintptr_t>(palette) & 15u) != 0)
        return fail(what, "a device palette must be 16-byte aligned");
    if (mo->nv == 0) return true;
    NR_CHECK(hipSetDevice(ctx->device));
    const f64 *dw = weights, *dpal = palette;
    if (!onDevice) {
        const size_t np = fused ? (size_t)s->nb * 12 : 0, nw = (size_t)mo->T;
        int slot = 0;
        f64* h = nr_mesh_pinned(ctx->tri, np + nw, &slot);
        if (!h) return fail(what, "hipHostMalloc failed");
        if (fused) std::memcpy(h, palette, np * sizeof(f64));
        std::memcpy(h + np, weights, nw * sizeof(f64));
        // (behind the kernels of earlier calls on this stream, which read the previous palette and weights)
        if (fused) NR_CHECK(hipMemcpyAsync(s->palette, h, np * sizeof(f64), hipMemcpyHostToDevice, ctx->stream));
        NR_CHECK(hipMemcpyAsync(mo->weights, h + np, nw * sizeof(f64), hipMemcpyHostToDevice, ctx->stream));
        NR_CHECK(hipEventRecord(ctx->tri.evMinst[slot], ctx->stream));
        dw = mo->weights;
        dpal = s ? s->palette : nullptr;
    }
    const bool nrm = m->lit && mo->normal != nullptr;
    if (!fused) {
        const i64 stride2 = mo->stride / 2;
        mesh_launch(ctx, NRK_MESH_MORPH, nrm ? k_mesh_morph<true> : k_mesh_morph<false>, stride2,
                    reinterpret_cast<const double2*>(mo->pos), reinterpret_cast<const double2*>(mo->normal),
                    reinterpret_cast<const double2*>(mo->dpos), reinterpret_cast<const double2*>(mo->dnormal), stride2,
                    dw, (u32)mo->T, mo->nv * 3, m->pos, m->normal);
        return true;
    }
    const bool lds = s->variant != 1 && s->nb <= (i64)SKIN_LDS_MAX_BONES;
    const auto kernel = lds ? (nrm ? k_mesh_morph_skin<true, true> : k_mesh_morph_skin<false, true>)
                            : (nrm ? k_mesh_morph_skin<true, false> : k_mesh_morph_skin<false, false>);
    mesh_launch(ctx, NRK_MESH_MORPH_SKIN, kernel, mo->nv, mo->pos, mo->normal, mo->dpos, mo->dnormal, mo->stride, dw,
                (u32)mo->T, reinterpret_cast<const uint4*>(s->joints), reinterpret_cast<const double2*>(s->weights),
                reinterpret_cast<const double2*>(dpal), (u32)s->nb, mo->nv, m->pos, m->normal);
    return true;
}

}  // namespace

extern "C" {

// New: nv base positions and T target-major position deltas (T*nv*3), and both or neither of base normals and
// normal deltas, uploaded once to the current device.  NULL + error (nothing allocated) for a negative or > 32-bit
// nv, T outside 1 .. 1024, a NULL positions array with nv > 0, or exactly one of the two normal arrays.  Nothing
// is validated beyond that.
MeshMorph* CreateMeshMorph(i64 nv, const f64* basePos, const f64* baseNormal, i64 T, const f64* deltaPos,
                           const f64* deltaNormal) {
    const char* what = "CreateMeshMorph";
    const char* why = nullptr;
    if (nv < 0) why = "negative vertex count";
    else if (nv > (i64)0xFFFFFFFFll) why = "vertex count beyond 32 bits";
    else if (T < 1) why = "the target count must be positive";
    else if (T > (i64)MORPH_MAX_TARGETS) why = "more than 1024 targets";
    else if ((baseNormal != nullptr) != (deltaNormal != nullptr)) why = "base normals and normal deltas go together";
    else if (nv > 0 && !basePos) why = "NULL base positions";
    else if (nv > 0 && !deltaPos) why = "NULL position deltas";
    if (why) {
        fail(what, why);
        return nullptr;
    }
    MeshMorph* mo = new MeshMorph();
    mo->nv = nv;
    mo->T = T;
    NR_CHECK(hipGetDevice(&mo->device));
    if (nv == 0) return mo;
    const i64 n3 = nv * 3;
    mo->stride = (n3 + 1) & ~(i64)1;
    const size_t row = (size_t)mo->stride * sizeof(f64);
    bool ok = hipMalloc(&mo->pos, row) == hipSuccess && hipMalloc(&mo->dpos, (size_t)T * row) == hipSuccess &&
              hipMalloc(&mo->weights, (size_t)T * sizeof(f64)) == hipSuccess;
    if (ok && baseNormal)
        ok = hipMalloc(&mo->normal, row) == hipSuccess && hipMalloc(&mo->dnormal, (size_t)T * row) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fail(what, "hipMalloc failed");
        free_morph(mo);
        return nullptr;
    }
    hipStream_t st = nr_stream_for(mo->device);
    const struct { f64* d; const f64* h; i64 rows; } parts[] = {
        {mo->pos, basePos, 1}, {mo->dpos, deltaPos, T}, {mo->normal, baseNormal, 1}, {mo->dnormal, deltaNormal, T}};
    for (const auto& p : parts) {
        if (!p.d) continue;
        if (mo->stride != n3) NR_CHECK(hipMemsetAsync(p.d, 0, (size_t)p.rows * row, st));   // (the padding: zero)
        upload_rows(p.d, p.h, p.rows, n3, mo->stride, st);
    }
    NR_CHECK(hipStreamSynchronize(st));   // caller may reuse its arrays on return
    return mo;
}

// Waits for the device's main stream (a morph kernel may still read the arrays), as DestroyMeshSkin does.
void DestroyMeshMorph(MeshMorph* mo) {
    if (!mo) return;
    int prev = 0;
    NR_CHECK(hipGetDevice(&prev));
    NR_CHECK(hipSetDevice(mo->device));
    NR_CHECK(hipStreamSynchronize(nr_stream_for(mo->device)));
    free_morph(mo);
    NR_CHECK(hipSetDevice(prev));
}

i64 GetMeshMorphTargetCount(MeshMorph* mo) { return mo->T; }

// New: morphs `m` under `weights` (T, host; the caller's again on return): its positions, and its normals when the
// mesh is lit and the morph has normals.  Draws issued before the call keep the old vertices, draws issued after
// it see the new ones; the host waits for nothing.
bool MorphMesh(RenderContext* ctx, Mesh* m, MeshMorph* mo, const f64* weights) {
    return morph(ctx, m, nullptr, nullptr, mo, weights, false, false, "MorphMesh");
}

// New: the same from device-resident weights (16-byte aligned; valid and unchanged until the call's kernel has
// executed, as PoseMeshDevice's palette).
bool MorphMeshDevice(RenderContext* ctx, Mesh* m, MeshMorph* mo, const f64* weights) {
    return morph(ctx, m, nullptr, nullptr, mo, weights, false, true, "MorphMeshDevice");
}

// New: morph, then skin, in one kernel: the morph's result takes the place of the skin's bind pose, which is not
// read.  The normals are written when the mesh is lit and the MORPH has normals.
bool PoseMeshMorphed(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette, MeshMorph* mo, const f64* weights) {
    return morph(ctx, m, s, palette, mo, weights, true, false, "PoseMeshMorphed");
}

bool PoseMeshMorphedDevice(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette, MeshMorph* mo,
                           const f64* weights) {
    return morph(ctx, m, s, palette, mo, weights, true, true, "PoseMeshMorphedDevice");
}

}  // extern "C"
