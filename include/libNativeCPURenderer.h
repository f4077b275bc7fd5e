/*
 * libNativeCPURenderer.h — C ABI of the MI355X (gfx950) raster library.
 *
 * Drop-in for the render part of the reference's ABI
 * (/root/reference/src/libNativeCPURenderer.h:83-152): the same symbol names
 * and parameter types (LP64: i64 = long, f64 = double, bool = C/C++ bool,
 * handles are opaque pointers), so the reference's ctypes binding
 * (libNativeCPURendererPybind.py) can load this .so unchanged for every raster
 * call.  Each declaration cites the reference prototype it replaces as
 * h:<line> and the implementation it restates as cpp:<lines>.
 *
 * Differences in behaviour: pixel data lives in HBM and draws
 * are asynchronous kernel launches — readback calls (GetBuffer*, GetColor,
 * GetDepthBuffer) and Flush are the sync points; Destroy* really free;
 * CreateRenderContext returns NULL when no HIP device is usable (no CPU path).
 * New entry points are additive and marked NEW.
 */
#ifndef LIBNATIVECPURENDERER_AMD_H
#define LIBNATIVECPURENDERER_AMD_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef long i64;
typedef double f64;
typedef unsigned char iu8;

typedef struct RenderContext RenderContext;   /* h:32-42 (opaque here) */
typedef struct Texture Texture;               /* h:44-49 (opaque here) */
typedef struct TriangleBuffer TriangleBuffer; /* NEW: device-resident triangle soup */

/* ---- render context (cpp:3-45, 277-316) ---------------------------------- */
i64 GetBufferSize(RenderContext* ctx);                                   /* h:84  */
RenderContext* CreateRenderContext(i64 width, i64 height, bool enableAlpha); /* h:85 */
void DestroyRenderContext(RenderContext* ctx);                           /* h:86  */
void ResizeRenderContext(RenderContext* ctx, i64 width, i64 height);     /* h:149 */
void SaveContextState(RenderContext* ctx);                               /* h:92  */
bool RestoreContextState(RenderContext* ctx);                            /* h:93  */
void GetBuffer(RenderContext* ctx, f64* buffer);                         /* h:94  */
void GetBufferAsUInt8(RenderContext* ctx, iu8* buffer);                  /* h:95  */

/* ---- textures (cpp:318-384, 950-988) ------------------------------------- */
Texture* CreateTexture(i64 width, i64 height, bool enableAlpha, f64* buffer);      /* h:96  */
Texture* CreateTextureUInt8(i64 width, i64 height, bool enableAlpha, iu8* buffer); /* h:97  */
void DestroyTexture(Texture* tex);                                       /* h:98  */
Texture* CreateTextureFromRenderContext(RenderContext* ctx);             /* h:99  */
Texture* CreateTextureFromRenderContextShared(RenderContext* ctx);       /* h:148 */
Texture* ResampleTexture(Texture* tex, i64 width, i64 height);           /* h:119 */
i64 GetTextureWidth(Texture* tex);                                       /* h:120 */
i64 GetTextureHeight(Texture* tex);                                      /* h:121 */
bool GetTextureEnableAlpha(Texture* tex);                                /* h:122 */

/* ---- audio clips (cpp:990-1283): interleaved f64 samples in HBM, ops as kernels */
typedef struct AudioClip AudioClip;           /* h:70-75 (opaque here) */
typedef struct WapperedBytes WapperedBytes;   /* h:77-80 (opaque here) */
i64 GetAudioClipBufferSizeFromData(i64 numFrames, i64 channels);          /* h:123 */
i64 GetAudioClipBufferSize(AudioClip* clip);                              /* h:124 */
AudioClip* CreateAudioClipFromBuffer(i64 sampleRate, i64 channels, i64 numFrames, f64* buffer); /* h:125 */
AudioClip* CreateAudioClipFromInt16Buffer(i64 sampleRate, i64 channels, i64 numFrames, short* buffer); /* h:126 */
AudioClip* CreateSilentAudioClip(i64 sampleRate, i64 channels, i64 numFrames); /* h:127 */
void DestroyAudioClip(AudioClip* clip);                                   /* h:128 (frees; a no-op there) */
AudioClip* CloneAudioClip(AudioClip* clip);                               /* h:129 */
void ApplyResampleAudioClip(AudioClip* clip, i64 sampleRate, i64 channels); /* h:130 */
void ResampleAudioClipLike(AudioClip* clip, AudioClip* like);             /* h:131 */
i64 OverlayAudioClip(AudioClip* target, AudioClip* source, i64 startFrame, bool autoResample); /* h:132;
                                                   0, -1 rate mismatch, -2 channel mismatch, -3 devices differ */
i64 OverlayAudioClipSecond(AudioClip* target, AudioClip* source, f64 startSecond, bool autoResample); /* h:133 */
WapperedBytes* SaveAudioClipAsWav(AudioClip* clip);                       /* h:134 */
i64 GetAudioClipSampleRate(AudioClip* clip);                              /* h:135 */
i64 GetAudioClipChannels(AudioClip* clip);                                /* h:136 */
i64 GetAudioClipNumFrames(AudioClip* clip);                               /* h:137 */
f64 GetAudioClipDuration(AudioClip* clip);                                /* h:138 */
iu8* GetWapperedBytesDataPtr(WapperedBytes* bytes);                       /* h:139 */
i64 GetWapperedBytesDataSize(WapperedBytes* bytes);                       /* h:140 */
void ApplyVolumeGain(AudioClip* clip, f64 gain);                          /* h:141 */
void ApplyCutAudioClip(AudioClip* clip, i64 startFrame, i64 endFrame);    /* h:144 */
void ApplySpeedAudioClip(AudioClip* clip, f64 speed);                     /* h:145 */
i64 OverlayAudioClipMany(AudioClip* target, AudioClip* source, const i64* startFrames, i64 n,
                         bool autoResample);  /* NEW: n OverlayAudioClip calls in order, one launch
                                                 (the note loop of milrenderer.py:810-815) */
i64 OverlayAudioClipManySecond(AudioClip* target, AudioClip* source, const f64* startSeconds, i64 n,
                               bool autoResample);  /* NEW: the same with OverlayAudioClipSecond times */
void DestroyWapperedBytes(WapperedBytes* bytes); /* NEW (the reference never frees them) */
void GetAudioClipBuffer(AudioClip* clip, f64* out); /* NEW: samples to the host */
void* GetAudioClipDevicePtr(AudioClip* clip);    /* NEW: samples in HBM (interop) */
void SetAudioStreamOrderedAlloc(bool on);        /* NEW (tests): clip buffers from hipMallocAsync/hipFreeAsync */

/* ---- texture preparation: procedural hit-effect shader (cpp:1318-1440) */
Texture* CreateMilthmHitEffectTexture(Texture* mask, f64 seed, f64 t, f64 r, f64 g, f64 b); /* h:151; NULL
                                                                   when the mask has no alpha (cpp:1418) */
void GetMilthmHitEffectPixel(f64 seed, f64 t, f64 x, f64 y, f64* a);     /* h:150 (inline there: not exported) */
bool CreateMilthmHitEffectTextures(Texture* mask, f64 seed, const f64* ts, i64 n, f64 r, f64 g, f64 b,
                                   Texture** out);  /* NEW: n thresholds ts[k] -> out[k], one launch
                                                       (Helpers.create_milthm_hit_effect_textures, Pybind:34-48) */

/* ---- transform / colour-transform state, host side (cpp:386-492, 623-641) */
void SetTransform(RenderContext* ctx, f64 a, f64 b, f64 c, f64 d, f64 e, f64 f);   /* h:100 */
void ApplyTransform(RenderContext* ctx, f64 a, f64 b, f64 c, f64 d, f64 e, f64 f); /* h:101 */
void Scale(RenderContext* ctx, f64 sx, f64 sy);                          /* h:102 */
void Translate(RenderContext* ctx, f64 tx, f64 ty);                      /* h:103 */
void Rotate(RenderContext* ctx, f64 angle);                              /* h:104 */
void TransformPoint(RenderContext* ctx, f64 x, f64 y, f64* out_x, f64* out_y); /* h:105 (inline in cpp:455; exported here) */
void GetTransform(RenderContext* ctx, f64 out_matrix[6]);                /* h:106 */
void GetInverseTransform(RenderContext* ctx, f64 out_matrix[6]);         /* h:107 */
void SetColorTransform(RenderContext* ctx, f64 r, f64 g, f64 b, f64 a);  /* h:110 */
void ApplyColorTransform(RenderContext* ctx, f64 r, f64 g, f64 b, f64 a); /* h:111 */

/* ---- pixel ops and primitives (cpp:494-948, 1285-1316) ------------------- */
bool SetPixel(RenderContext* ctx, i64 x, i64 y, f64 r, f64 g, f64 b, f64 a);   /* h:108 */
bool ApplyPixel(RenderContext* ctx, i64 x, i64 y, f64 r, f64 g, f64 b, f64 a); /* h:109 (inline in cpp:515; exported here) */
void SetColor(RenderContext* ctx, f64 r, f64 g, f64 b, f64 a);           /* h:112 */
void GetColor(RenderContext* ctx, f64 x, f64 y, f64* out_r, f64* out_g, f64* out_b, f64* out_a); /* h:113 */
void FillColor(RenderContext* ctx, f64 r, f64 g, f64 b, f64 a);          /* h:114 */
void DrawTexture(RenderContext* ctx, Texture* tex, f64 x, f64 y, f64 width, f64 height); /* h:115 */
void DrawRect(RenderContext* ctx, f64 x, f64 y, f64 width, f64 height, f64 r, f64 g, f64 b, f64 a); /* h:116 */
void DrawLine(RenderContext* ctx, f64 x1, f64 y1, f64 x2, f64 y2, f64 width,
              f64 r, f64 g, f64 b, f64 a);                               /* h:117 */
void DrawCircle(RenderContext* ctx, f64 x, f64 y, f64 radius, f64 r, f64 g, f64 b, f64 a); /* h:118 */
void DrawVerticalGrd(RenderContext* ctx, f64 x, f64 y, f64 width, f64 height,
                     f64 top_r, f64 top_g, f64 top_b, f64 top_a,
                     f64 bottom_r, f64 bottom_g, f64 bottom_b, f64 bottom_a); /* h:146 */
void DrawSplittedTexture(RenderContext* ctx, Texture* tex, f64 x, f64 y, f64 width, f64 height,
                         f64 uStart, f64 uEnd, f64 vStart, f64 vEnd);    /* h:147 */
i64 GetVersion(void);                                                     /* h:143, =1 (h:9) */

/* ---- NEW: triangles, depth, Gouraud (the north-star path) --
 * xy: n*6 f64 (x0,y0,x1,y1,x2,y2) in user space (the context transform is
 * applied); z: n*3 f64 depths in [0,1] or NULL; rgba: n*4 f64 flat colours,
 * or n*12 per-vertex colours when gouraud. */
void SetDepthState(RenderContext* ctx, bool test, bool write);           /* NEW: LESS test, write enable */
void ClearDepth(RenderContext* ctx, uint32_t value);                     /* NEW: deferred, on-chip */
void GetDepthBuffer(RenderContext* ctx, uint32_t* out);                  /* NEW: W*H u32, sync */
void DrawTriangles(RenderContext* ctx, const f64* xy, const f64* z, const f64* rgba,
                   i64 n, bool gouraud);                                  /* NEW: host arrays */
void DrawTrianglesDevice(RenderContext* ctx, const f64* xy, const f64* z, const f64* rgba,
                         i64 n, bool gouraud);                            /* NEW: device pointers; keep them valid
                                 and unchanged until the batch has executed (Flush / readback / device sync) */
TriangleBuffer* CreateTriangleBuffer(i64 n, const f64* xy, const f64* z, const f64* rgba,
                                     bool gouraud);                       /* NEW: one H2D upload */
void DestroyTriangleBuffer(TriangleBuffer* tb);                          /* NEW */
void DrawTriangleBuffer(RenderContext* ctx, TriangleBuffer* tb);         /* NEW */
i64 GetTriangleBufferCount(TriangleBuffer* tb);                          /* NEW */
/* NEW: textured triangles.  uv: n*6 per-vertex texture coordinates in texel units (u0 v0 u1 v1 u2 v2),
   interpolated like a Gouraud channel (affine) and sampled with DrawTexture's nearest sampler (a NaN
   coordinate samples texel 0) or, by SetTriangleTextureFilter, bilinearly; blended by ApplyPixel.  A NULL texture, one narrower or lower than 2
   texels, or one on another device latches an error and draws nothing. */
void DrawTexturedTriangles(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uv,
                           i64 n);                                        /* NEW: host arrays */
void DrawTexturedTrianglesDevice(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uv,
                                 i64 n);                                  /* NEW: device pointers (as DrawTrianglesDevice) */
/* NEW: perspective-correct textured triangles (DESIGN §3 "Perspective-correct texture mapping").  q: n*3, laid
   out like z, each corner's 1/w.  Per triangle a_k = u_k * q_k, b_k = v_k * q_k; per fragment U, V, Q are
   interpolated from a, b, q like a Gouraud channel and the texel is that of (U * (1 / Q), V * (1 / Q)).  q is
   not validated (a zero, negative or non-finite q gives a defined texel); q all 1 gives DrawTexturedTriangles'
   frame bit for bit; depth stays affine.  A NULL q latches an error and draws nothing; every texture check of
   DrawTexturedTriangles applies. */
void DrawTexturedTrianglesPerspective(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uv,
                                      const f64* q, i64 n);               /* NEW: host arrays */
void DrawTexturedTrianglesPerspectiveDevice(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z,
                                            const f64* uv, const f64* q, i64 n);   /* NEW: device pointers (as
                                 DrawTrianglesDevice) */
/* NEW: modulated textured triangles -- texel times vertex colour (DESIGN §3 "Modulated textured draws").  uvc:
   n*18, per corner k = 0..2 (u_k, v_k, r_k, g_k, b_k, A_k): a texel-unit UV and a colour; q: n*3 as above (all
   1.0 for affine mapping: there is no separate affine form).  With I(x) = x0 + (x1 - x0)*w1 + (x2 - x0)*w2, the
   Gouraud-channel expression on the raster's own barycentrics, per covered fragment, in f64, every operation
   rounded in the order written:
       a_k = u_k * q_k;  b_k = v_k * q_k                      (per triangle, as the perspective mode)
       U = I(a), V = I(b), Q = I(q);  rq = 1.0 / Q;  u = U * rq;  v = V * rq
       T = texel at (u, v) by the context's filter (nearest, or bilinear), unchanged; the alpha of a texture
           without alpha is the literal 1.0
       G_c = I(c)  for c in r, g, b, A
       src_c = T_c * G_c                                      (one rounded product per channel)
       ApplyPixel(src) as every triangle draw (colour transform, blend); depth as every triangle draw
   A NaN stays a NaN (payload bits unspecified); q is not validated.  Every colour (1, 1, 1, 1) gives
   DrawTexturedTrianglesPerspective's frame; a texture of texels all 1.0 under the nearest filter gives the Gouraud
   DrawTriangles frame of those colours.  The batch takes the order-free raster exactly when the texture has no
   alpha, every A_k == 1, the colour transform's alpha is 1 and the ordered raster is not forced.  A NULL uvc or a
   NULL q latches an error under the entry point's name and draws nothing; every texture check of
   DrawTexturedTriangles applies. */
void DrawTexturedTrianglesModulated(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z, const f64* uvc,
                                    const f64* q, i64 n);                 /* NEW: host arrays */
void DrawTexturedTrianglesModulatedDevice(RenderContext* ctx, Texture* tex, const f64* xy, const f64* z,
                                          const f64* uvc, const f64* q, i64 n);   /* NEW: device pointers (as
                                 DrawTrianglesDevice: xy / uvc re-staged when not 16-byte aligned, z and q the caller's) */
TriangleBuffer* CreateTexturedTriangleBuffer(i64 n, const f64* xy, const f64* z,
                                             const f64* uv);              /* NEW: one H2D upload; no texture bound */
void DrawTexturedTriangleBuffer(RenderContext* ctx, TriangleBuffer* tb, Texture* tex);   /* NEW: texture chosen per
                                 draw; a colour buffer here, or a textured one in DrawTriangleBuffer, latches an error */
/* NEW: the texture filter of the textured triangle draws (DESIGN §3 "Bilinear texture filtering"): 0 nearest (the
   default), 1 bilinear -- the filter in the body of the reference's sampler, restated bit for bit: (u, v) clamped
   as the nearest sampler clamps it, the texels (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1) weighted by the
   fractions in f64, every operation rounded in the order written; the alpha of a texture without alpha stays the
   literal 1.  It covers DrawTexturedTriangles and its Device / Perspective variants, DrawTexturedTriangleBuffer
   and DrawTexturedMesh; colour draws, DrawTexture, DrawSplittedTexture and ResampleTexture are untouched.  Per
   context, not saved / restored, not recorded; read when a draw is issued (a pending batch keeps its filter).
   Any other mode latches an error, leaves the state unchanged and returns false. */
bool SetTriangleTextureFilter(RenderContext* ctx, i64 mode);             /* NEW */
i64 GetTriangleTextureFilter(RenderContext* ctx);                        /* NEW */
/* NEW: the wrap addressing of the textured triangle draws (DESIGN §3 "Wrap addressing"), per axis: 0 clamp (the
   default: the samplers above), 1 repeat, 2 mirrored repeat.  Per axis (columns: n = w, x = u; rows: n = h, x = v),
   with P = (f64)n for repeat and (f64)(2n) for mirror, in f64, every operation rounded in the order written, the
   divide IEEE:
       k = floor(x / P);  t = x - k * P;  if !(t >= 0) t = 0;  if (t >= P) t = 0
       i0 = (i64)t;  f = t - i0;  i1 = i0 + 1, or 0 when that is P
       c(j) = j (repeat);  c(j) = j < n ? j : 2n - 1 - j (mirror)
   The nearest filter takes texel c(i0); the bilinear filter c(i0) and c(i1) with weights 1 - f and f.  The axes are
   independent: one may clamp while the other wraps.  Texel centres stay on the integer lattice (no half-texel
   offset), so a seamless tile needs no duplicated edge texel.  Every coordinate (NaN, infinite, huge, negative)
   gives in-range texels; nothing is validated.  For x in [0, n-1) all three modes give the same footprint.  It
   covers everything SetTriangleTextureFilter covers and the Modulated, MeshInstanced and MeshLit textured draws;
   colour draws, DrawTexture, DrawSplittedTexture and ResampleTexture are untouched.  Per context, not saved /
   restored, not recorded; read when a draw is issued (a pending batch keeps its state).  A mode outside 0..2 on
   either axis latches an error, leaves both axes unchanged and returns false. */
bool SetTriangleTextureWrap(RenderContext* ctx, i64 modeU, i64 modeV);   /* NEW */
void GetTriangleTextureWrap(RenderContext* ctx, i64* modeU, i64* modeV); /* NEW */
/* NEW: indexed 3D meshes (DESIGN §3 "Vertex stage").  nv vertices pos (px, py, pz), n triangles as u32 index
   triples, one per-vertex attribute: RGBA nv*4 (flat = the colour of a triangle's first index, or Gouraud) or
   texel-unit UVs nv*2.  Uploaded once; each draw transforms the vertices on the device by a row-major 4x4
   matrix16 with the viewport baked in (NULL = identity): c = M * (px, py, pz, 1), a vertex with cw <= 0 becomes
   NaN (its triangles are dropped; no near-plane clipping), otherwise (x, y, z) = (cx, cy, cz) / cw.  The assembled
   soup is then drawn like DrawTrianglesDevice's: the context's 2D transform, depth state and colour transform
   apply, attributes stay affine in screen space (a textured mesh: unless SetMeshPerspective is on).  Creation returns NULL and latches an error for an index >= nv,
   a NULL attribute array with n > 0, or nv beyond 32 bits; n == 0 is a valid mesh that draws nothing.  A mesh on
   another device than the context's, or the wrong draw call for its kind, latches an error and draws nothing. */
typedef struct Mesh Mesh;
Mesh* CreateMesh(i64 nv, const f64* pos, i64 n, const uint32_t* idx, const f64* rgba, bool gouraud);   /* NEW */
Mesh* CreateTexturedMesh(i64 nv, const f64* pos, i64 n, const uint32_t* idx, const f64* uv);           /* NEW */
void DestroyMesh(Mesh* m);                                               /* NEW */
i64 GetMeshVertexCount(Mesh* m);                                         /* NEW */
i64 GetMeshTriangleCount(Mesh* m);                                       /* NEW */
bool UpdateMeshPositions(Mesh* m, const f64* pos);                       /* NEW: deforming meshes, H2D of nv*3 positions only */
void DrawMesh(RenderContext* ctx, Mesh* m, const f64* matrix16);         /* NEW: a colour mesh */
void DrawTexturedMesh(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrix16);   /* NEW: texture chosen per draw */
bool AssembleMesh(RenderContext* ctx, Mesh* m, const f64* matrix16, f64* xy_out, f64* z_out);   /* NEW: DrawMesh's
                                 vertex stage and assembly alone, the soup (xy n*6, z n*3) copied to the host; a sync point */
/* NEW: near-plane clipping and back-face culling of mesh draws (DESIGN §3 "Clip stage").  Per context, not part
   of the save / restore stack, not recorded in command lists.  With both off (the default) mesh draws are
   unchanged.  With either on, a mesh draw clips every triangle against cw = wNear on the device (0, 1 or 2 output
   triangles, attributes interpolated in clip space, submission order kept), culls each output triangle by the
   sign of area2 = (x1-x0)*(y2-y0) - (x2-x0)*(y1-y0) before the context's 2D transform (zero and NaN areas are
   never culled), reads the output count back -- one wait for the device, of such draws only -- and rasterises
   exactly that many triangles.  AssembleMesh ignores the state. */
bool SetMeshNearPlane(RenderContext* ctx, f64 wNear);                    /* NEW: 0 off, > 0 the plane; negative or
                                 non-finite: false, error latched, state unchanged */
f64 GetMeshNearPlane(RenderContext* ctx);                                /* NEW */
bool SetMeshCull(RenderContext* ctx, i64 mode);                          /* NEW: 0 none, 1 drops area2 > 0, 2 drops
                                 area2 < 0; another value: false, error latched, state unchanged */
i64 GetMeshCull(RenderContext* ctx);                                     /* NEW */
i64 GetMeshLastTriangleCount(RenderContext* ctx);                        /* NEW: triangles the last mesh draw of ctx
                                 rasterised: n_out of the clip stage, the mesh's n when the stage was off */
bool AssembleMeshClipped(RenderContext* ctx, Mesh* m, const f64* matrix16, i64 cap, f64* xy_out, f64* z_out,
                         f64* attr_out, i64* n_out);                     /* NEW: the soup a draw of m rasterises under
                                 ctx's near plane and cull mode (the draw's own kernels): the full count in *n_out, the
                                 first min(cap, *n_out) triangles copied to the host (xy x6, z x3, attr x12 Gouraud / x4
                                 flat / x6 textured); a sync point; either mesh kind */
/* NEW: perspective-correct texture mapping of DrawTexturedMesh.  Per context, off by default, not
   part of the save / restore stack, not recorded in command lists.  On: the vertex stage keeps q = 1.0 / cw per
   vertex (NaN where cw <= 0; a cut vertex of the clip stage: 1.0 / wNear) and the draw is a
   DrawTexturedTrianglesPerspective batch; under a matrix whose last row is (0, 0, 0, 1) q == 1 and the frame is
   the state-off frame bit for bit.  DrawMesh of a colour mesh ignores the state: colours stay affine. */
bool SetMeshPerspective(RenderContext* ctx, bool on);                    /* NEW: returns true */
bool GetMeshPerspective(RenderContext* ctx);                             /* NEW */
bool AssembleMeshPerspective(RenderContext* ctx, Mesh* m, const f64* matrix16, i64 cap, f64* xy_out, f64* z_out,
                             f64* uv_out, f64* q_out, i64* n_out);       /* NEW: the soup a DrawTexturedMesh of m
                                 rasterises under ctx's near plane, cull mode and perspective state (the draw's own
                                 kernels): the full count in *n_out, the first min(cap, *n_out) triangles copied to the
                                 host (xy x6, z x3, uv x6, q x3; q is 1.0 with the state off); a sync point; a textured
                                 mesh only */
/* NEW: instanced mesh draws (DESIGN §3 "Instanced mesh draws"): one mesh under K row-major 4x4 matrices (K*16) as
   ONE batch -- by definition the frame of K DrawMesh / DrawTexturedMesh calls in instance order (triangle t of
   instance k is triangle k*n + t of the batch), from one vertex and assembly pass and one binning.  Every state
   of DrawMesh applies unchanged (transform, depth, colour transform, near plane, cull, perspective, filter,
   sharding); GetMeshLastTriangleCount is the batch's total.  tint: K*4 (r, g, b, a) or NULL -- every vertex colour
   of instance k times tint[k] (one rounded product, before anything else); NULL: no product.  A textured mesh
   takes no tint.  K == 0 draws nothing; K < 0, NULL matrices with K > 0, a tint on a textured mesh, or more than
   2^31 - 1 triangles (K*n) or vertices (K*nv): error latched, nothing drawn, the last count 0. */
void DrawMeshInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* tint, i64 K);   /* NEW: host
                                 arrays, the caller's again on return */
void DrawTexturedMeshInstanced(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrices, i64 K);   /* NEW */
void DrawMeshInstancedDevice(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* tint, i64 K);   /* NEW:
                                 device pointers, valid and unchanged until the draw has executed (as
                                 DrawTrianglesDevice); read only by kernels launched inside the call */
void DrawTexturedMeshInstancedDevice(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrices, i64 K);   /* NEW */
bool AssembleMeshInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* tint, i64 K, i64 cap,
                           f64* xy_out, f64* z_out, f64* attr_out, f64* q_out, i64* n_out);   /* NEW: the soup an
                                 instanced draw of m rasterises under ctx's near plane, cull mode and perspective
                                 state (the draw's own kernels; host matrices and tint): the full count in *n_out, the
                                 first min(cap, *n_out) triangles copied to the host (xy x6, z x3, attr x12 / x4 / x6;
                                 q x3 only for a perspective textured draw, q_out may be NULL otherwise); a sync
                                 point; either mesh kind */
/* NEW: lit meshes (DESIGN §3 "Vertex lighting"): per-vertex normals under an ambient colour and up to 8
   directional lights, computed on the device by one pass over the vertices of each *Lit draw.  Per vertex, in
   f64, every product and sum rounded in the order written (no sqrt, no division, no renormalisation: unit normals
   and rotation-only normal matrices are the caller's business), with N the row-major 3x3 normal matrix:
     wx = (N[0]*nx + N[1]*ny) + N[2]*nz   (wy: row 1, wz: row 2);   acc_c = ambient_c;
     per light (dx, dy, dz, cr, cg, cb) in order, d towards the light:
       dot = (wx*dx + wy*dy) + wz*dz;  d = dot > 0 ? dot : 0.0 (a NaN dot: 0);  acc_c = acc_c + d * c_c;
     lit_c = clamp(base_c * acc_c) to [0, 1] (a NaN stays NaN);  alpha is untouched.
   The lit colours replace the mesh's own before anything else reads them: a flat mesh takes the lit colour of a
   triangle's first index, the clip stage interpolates lit colours, an instance's tint multiplies them.  Every
   state of DrawMesh applies, and with the default lights (ambient (1, 1, 1), none) a lit draw is DrawMesh's frame
   bit for bit.  The light state is per context, copied at the call, not part of the save / restore stack, not
   recorded in command lists, and read when a draw is issued.  A *Lit call with a mesh that has no normals, or a
   textured mesh: error latched, nothing drawn, the last count 0. */
Mesh* CreateLitMesh(i64 nv, const f64* pos, const f64* normal, i64 n, const uint32_t* idx, const f64* rgba,
                    bool gouraud);                                       /* NEW: CreateMesh with normals (nv*3); NULL
                                 normals with nv > 0: NULL, error latched.  DrawMesh / DrawMeshInstanced draw it unlit */
bool UpdateMeshNormals(Mesh* m, const f64* normal);                      /* NEW: as UpdateMeshPositions; a mesh without
                                 normals: false, error latched */
bool GetMeshLit(Mesh* m);                                                /* NEW: created with normals */
bool SetMeshLights(RenderContext* ctx, const f64* ambient3, const f64* lights, i64 nl);   /* NEW: ambient3 NULL:
                                 (1, 1, 1); lights nl*6, 0 <= nl <= 8; nl out of range or NULL lights with nl > 0:
                                 false, error latched, state unchanged; the values are not validated */
i64 GetMeshLightCount(RenderContext* ctx);                               /* NEW */
void DrawMeshLit(RenderContext* ctx, Mesh* m, const f64* matrix16, const f64* normal9);   /* NEW: normal9 NULL: the
                                 identity */
void DrawMeshLitInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* normals, const f64* tint,
                          i64 K);                                        /* NEW: normals K*9 or NULL (the identity for
                                 every instance), tint K*4 or NULL; DrawMeshInstanced's checks and limits; host
                                 arrays, the caller's again on return */
void DrawMeshLitInstancedDevice(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* normals,
                                const f64* tint, i64 K);                 /* NEW: device pointers, valid and unchanged
                                 until the draw has executed; read only by kernels launched inside the call */
bool AssembleMeshLit(RenderContext* ctx, Mesh* m, const f64* matrix16, const f64* normal9, i64 cap, f64* xy_out,
                     f64* z_out, f64* attr_out, i64* n_out);             /* NEW: the soup a DrawMeshLit rasterises under
                                 ctx's lights, near plane and cull mode (the draw's own kernels), in
                                 AssembleMeshClipped's conventions (attr x12 Gouraud / x4 flat); a sync point */
/* NEW: textured colour meshes -- lit, textured, posed (DESIGN §3 "Modulated textured draws").  A mesh with both a
   texel-unit uv (nv*2) and a colour (nv*4) per vertex, and normals (nv*3) or NULL (GetMeshLit).  It keeps the
   per-vertex uv and rgba on the device; its expanded attributes are n*18, per corner (u, v, r, g, b, a).
   DrawTexturedMesh draws it as a DrawTexturedTrianglesModulated batch, modulated by its own colours, unlit;
   DrawTexturedMeshLit first runs the light pass of DrawMeshLit on the colours (the uv untouched).  Every state of
   DrawTexturedMesh applies (transform, depth, colour transform, filter, near plane, cull, SetMeshPerspective,
   sharding, GetMeshLastTriangleCount): the clip stage interpolates all six attribute values in clip space, a cut
   vertex has q = 1 / wNear, and with the perspective state off every q is 1.0.  With the default lights and colours
   in [0, 1] the lit draw is the unlit draw bit for bit.  UpdateMeshPositions, UpdateMeshNormals, PoseMesh and
   GetMeshNormals work on it as on a lit colour mesh.  DrawMesh, DrawMeshLit, every *Instanced draw and the other
   Assemble* calls (AssembleMesh apart) latch "not supported for a textured colour mesh" and draw nothing;
   DrawTexturedMeshLit on another kind of mesh, or on one without normals, latches an error, draws nothing and
   sets the last count to 0. */
Mesh* CreateTexturedColorMesh(i64 nv, const f64* pos, const f64* normal, i64 n, const uint32_t* idx, const f64* uv,
                              const f64* rgba);                          /* NEW: normal nv*3 or NULL; CreateMesh's
                                 checks, and NULL uv or rgba with n > 0 */
void DrawTexturedMeshLit(RenderContext* ctx, Mesh* m, Texture* tex, const f64* matrix16, const f64* normal9);   /* NEW */
bool AssembleTexturedColorMesh(RenderContext* ctx, Mesh* m, const f64* matrix16, const f64* normal9, bool lit, i64 cap,
                               f64* xy_out, f64* z_out, f64* uvc_out, f64* q_out, i64* n_out);   /* NEW: the soup such
                                 a draw rasterises (the draw's own kernels), in AssembleMeshPerspective's conventions
                                 (uvc x18, q x3); lit false: DrawTexturedMesh's, normal9 ignored; a sync point */
bool AssembleMeshLitInstanced(RenderContext* ctx, Mesh* m, const f64* matrices, const f64* normals, const f64* tint,
                              i64 K, i64 cap, f64* xy_out, f64* z_out, f64* attr_out, i64* n_out);   /* NEW: the same
                                 for a DrawMeshLitInstanced, in AssembleMeshInstanced's conventions without q */
/* NEW: skinned meshes (DESIGN §3 "Skinned meshes"): linear-blend skinning on the device.  A MeshSkin keeps a bind
   pose -- nv positions, optionally nv normals, four joints (u32) and four weights (f64) per vertex, for nb bones --
   and PoseMesh rewrites a mesh's positions (and normals) from it under a palette of nb row-major 3x4 matrices
   [R | t], 12 doubles each, by one kernel.  Per vertex, in f64, every product and sum rounded in the order written
   (no FMA, no division, no sqrt, no renormalisation), with B_k = palette[j_k], k = 0 .. 3, all four evaluated:
     x_k = ((B_k[0]*px + B_k[1]*py) + B_k[2]*pz) + B_k[3]   (y_k: entries 4..7, z_k: entries 8..11)
     X   = ((w0*x_0 + w1*x_1) + w2*x_2) + w3*x_3            (Y, Z likewise)
     a_k = (B_k[0]*nx + B_k[1]*ny) + B_k[2]*nz              (b_k: entries 4..6, c_k: entries 8..10; no translation)
     NX  = ((w0*a_0 + w1*a_1) + w2*a_2) + w3*a_3            (NY, NZ likewise)
   Posing always starts from the bind pose.  Weights are not validated; every joint, zero-weight ones included,
   must be < nb (checked at creation).  The normals are rewritten when the mesh is lit AND the skin has bind
   normals; otherwise a lit mesh keeps its own.  Draws issued before a Pose call keep the old pose, draws issued
   after it see the new one, on any context of the device, and the host waits for nothing.  Every existing mesh
   draw works on the posed mesh unchanged.  Each error latches a message under the entry point's name and changes
   nothing: NULL arguments, nb <= 0 or beyond 32 bits, a joint >= nb, a mesh and a skin of different vertex counts,
   mesh, skin and context not all on one device.  nv == 0 is valid and does nothing. */
typedef struct MeshSkin MeshSkin;
MeshSkin* CreateMeshSkin(i64 nv, const f64* bindPos, const f64* bindNormal, const uint32_t* joints,
                         const f64* weights, i64 nb);                    /* NEW: bindNormal NULL: positions only;
                                 joints and weights nv*4; host arrays, the caller's again on return */
void DestroyMeshSkin(MeshSkin* s);                                       /* NEW: waits for the device's stream */
i64 GetMeshSkinBoneCount(MeshSkin* s);                                   /* NEW */
void SetMeshSkinVariant(MeshSkin* s, i64 mode);                          /* NEW (A/B and tests): the skin kernel 0 auto,
                                 1 palette from global memory, 2 staged in LDS (nb <= 128); the same bits */
bool PoseMesh(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette);   /* NEW: host palette nb*12, the
                                 caller's again on return (one asynchronous copy through a pinned buffer) */
bool PoseMeshDevice(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette);   /* NEW: device pointer, 16-byte
                                 aligned, valid and unchanged until the call's kernel has executed; read only by it */
bool GetMeshPositions(Mesh* m, f64* out);                                /* NEW: nv*3 to the host; a sync point */
bool GetMeshNormals(Mesh* m, f64* out);                                  /* NEW: a lit mesh only (else false, error
                                 latched) */
/* NEW: morph targets (DESIGN §3 "Morph targets"): blend shapes on the device, alone or fused with skinning.  A
   MeshMorph keeps nv base positions and T (1 .. 1024) target-major position deltas dP[t][v] (T*nv*3), and either
   both or neither of base normals and normal deltas dN[t][v].  A call supplies T weights and one kernel rewrites
   the mesh's positions (and normals).  Per vertex and component, in f64, every product and sum rounded in the order
   written (no FMA, no division, no renormalisation):
     X = px;  for t = 0 .. T-1 in index order:  if w_t == 0.0 skip the target;  X = X + w_t * dPx[t][v]
   (Y, Z, and NX, NY, NZ from the base normal and dN, likewise).  The skip is part of the definition: a target under
   a zero weight of either sign contributes nothing, NaN or infinite deltas included, and with every weight zero the
   result is the base bit for bit; a NaN weight is not zero.  Weights and deltas are not validated.
   PoseMeshMorphed evaluates this in registers and feeds the result to PoseMesh's expressions in place of the skin's
   bind position and normal (the skin's own bind arrays are not read): it equals MorphMesh, a read-back, a skin
   created with that as its bind pose and PoseMesh, bit for bit.  Positions are always written; normals when the
   mesh is lit AND the morph has normals (fused: whether or not the skin has bind normals); otherwise a lit mesh
   keeps its own.  PoseMesh after MorphMesh starts from the skin's bind pose, as always, and overwrites the morph.
   Ordering is PoseMesh's: draws issued before a call keep the old vertices, draws issued after it see the new ones,
   on any context of the device, and the host waits for nothing.  Each error latches a message under the entry
   point's name and changes nothing: NULL arguments, nv < 0 or beyond 32 bits, T < 1 or > 1024, exactly one of
   baseNormal / deltaNormal, mesh, morph and skin of different vertex counts, objects not all on one device, a
   device pointer that is not 16-byte aligned.  nv == 0 is valid and does nothing. */
typedef struct MeshMorph MeshMorph;
MeshMorph* CreateMeshMorph(i64 nv, const f64* basePos, const f64* baseNormal, i64 T, const f64* deltaPos,
                           const f64* deltaNormal);                      /* NEW: host arrays, the caller's again on
                                 return; baseNormal and deltaNormal both NULL: positions only */
void DestroyMeshMorph(MeshMorph* mo);                                    /* NEW: waits for the device's stream */
i64 GetMeshMorphTargetCount(MeshMorph* mo);                              /* NEW */
bool MorphMesh(RenderContext* ctx, Mesh* m, MeshMorph* mo, const f64* weights);   /* NEW: host weights T, the
                                 caller's again on return (one asynchronous copy through a pinned buffer) */
bool MorphMeshDevice(RenderContext* ctx, Mesh* m, MeshMorph* mo, const f64* weights);   /* NEW: device pointer,
                                 16-byte aligned, valid and unchanged until the call's kernel has executed */
bool PoseMeshMorphed(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette, MeshMorph* mo,
                     const f64* weights);                                /* NEW: morph then skin in one kernel; host
                                 palette nb*12 and weights T, through ONE pinned buffer */
bool PoseMeshMorphedDevice(RenderContext* ctx, Mesh* m, MeshSkin* s, const f64* palette, MeshMorph* mo,
                           const f64* weights);                          /* NEW: palette and weights both device
                                 pointers, 16-byte aligned, under PoseMeshDevice's lifetime rule */
void SetFragmentCounting(RenderContext* ctx, bool on);                   /* NEW: covered-fragment counter */
i64 GetFragmentCount(RenderContext* ctx);                                /* NEW */
i64 GetLastRasterPath(RenderContext* ctx);                               /* NEW: 1 order-free tiled, 2 ordered */
void SetForceOrderedRaster(RenderContext* ctx, bool on);                 /* NEW: A/B and tests */
void SetPairCapacityOverride(RenderContext* ctx, i64 pairs);             /* NEW: tests (0 = automatic) */
void SetCoopRaster(RenderContext* ctx, i64 mode);                        /* NEW: k_vis variant 0 auto, 1 coop, 2 lane-only */
void SetWarmBinning(RenderContext* ctx, i64 mode);                       /* NEW: one-pass binning of a repeat draw 0 auto, 1 on, 2 off */
i64 GetWarmBatchCount(RenderContext* ctx);                               /* NEW (testing): batches binned warm */
i64 GetLooseBatchCount(RenderContext* ctx);                              /* NEW (testing): of those, binned into the loose
                                                                            ranges of a changed transform */
i64 GetReusedBatchCount(RenderContext* ctx);                             /* NEW (testing): of the warm batches, rasterised
                                                                            from a kept pair list (no binning) */
void SetListReuse(RenderContext* ctx, i64 mode);                         /* NEW: pair-list reuse of an unchanged repeat draw
                                                                            0 auto (on), 2 off (every warm batch bins) */
i64 GetPrunedBatchCount(RenderContext* ctx);                             /* NEW (testing): of the reused batches, rasterised
                                                                            from the visible list (no hidden triangles) */
i64 GetVisiblePairCount(RenderContext* ctx);                             /* NEW (testing): pairs kept in the current visible
                                                                            list, 0 when there is none */
void SetVisiblePruning(RenderContext* ctx, i64 mode);                    /* NEW: visible list of an unchanged repeat draw
                                                                            0 auto (on), 2 off (reuse the full list) */
void SetVisibleReplan(RenderContext* ctx, i64 mode);                     /* NEW: work items of the visible list planned from
                                                                            its kept counts, 0 auto (on), 2 off (the
                                                                            schedule's items over the pruned list) */
i64 GetReplannedBatchCount(RenderContext* ctx);                          /* NEW (testing): of the pruned batches, rasterised
                                                                            under the visible plan */
bool GetVisiblePlanTotals(RenderContext* ctx, i64* out4);                /* NEW (testing): the visible plan's kept pairs, work
                                                                            items, split-tile slices, dense tiles; false:
                                                                            none.  Waits for the device */
void SetKeyCache(RenderContext* ctx, i64 mode);                          /* NEW: an unchanged repeat draw shaded from its cached
                                                                            visibility keys, 0 auto (on), 2 off (the visible
                                                                            list; the cached keys are kept) */
i64 GetKeyCachedBatchCount(RenderContext* ctx);                          /* NEW (testing): of the pruned batches, shaded from
                                                                            the key cache (no raster) */
bool GetKeyCacheTotals(RenderContext* ctx, i64* out3);                   /* NEW (testing): the key cache's cached tiles, key
                                                                            items, bytes of keys; false: none.  Waits for
                                                                            the device */
void SetKeyIndex(RenderContext* ctx, i64 mode);                          /* NEW: a cached Gouraud draw shaded from its tiles'
                                                                            winner index, 0 auto (on), 2 off (the cached keys
                                                                            alone; the index is kept) */
i64 GetKeyIndexedBatchCount(RenderContext* ctx);                         /* NEW (testing): of the cached batches, shaded from
                                                                            the key index */
bool GetKeyIndexTotals(RenderContext* ctx, i64* out4);                   /* NEW (testing): the key index's tiles, staged
                                                                            winners, directly loaded pixels, bytes; false:
                                                                            none.  Waits for the device */
void SetKeyRecords(RenderContext* ctx, i64 mode);                        /* NEW: an indexed Gouraud draw shaded from its winners'
                                                                            shading records, built once per generation, 0 auto
                                                                            (on), 2 off (the key index; the records are kept) */
i64 GetKeyRecordBatchCount(RenderContext* ctx);                          /* NEW (testing): of the indexed batches, shaded from
                                                                            the key records */
bool GetKeyRecordTotals(RenderContext* ctx, i64* out3);                  /* NEW (testing): the key records' slots, records,
                                                                            bytes; false: none.  Waits for the device */
void SetDeferredStores(RenderContext* ctx, i64 mode);                    /* NEW: a cached Gouraud draw that writes the frame
                                                                            output leaves its f64 and depth stores pending
                                                                            until the buffers are used: 0 auto (only after
                                                                            frames whose values nothing needed), 1 always,
                                                                            2 off */
void GetDeferredStoreCounts(RenderContext* ctx, i64* out4);              /* NEW (testing): batches deferred, resolves
                                                                            launched, records superseded unread, the rule's
                                                                            threshold.  Host state: no device wait */
bool GetScheduleTotals(RenderContext* ctx, i64* out4);                  /* NEW (testing): the warm schedule's pairs, work
                                                                            items, split-tile slices, dense tiles; false: none */
void SetWarmFaultInjection(RenderContext* ctx, i64 mode);                /* NEW (testing): fault in the next warm batch
                                 1 range overflow, 2 withheld token, 3 dropped pairs, 4 binning delayed past the
                                 raster's token wait (the frame must stay exact) */
i64 GetWarmFailureCount(RenderContext* ctx);                             /* NEW (testing): warm batches that failed a check */
void SetSplitLimits(RenderContext* ctx, i64 splitAt, i64 dslice);       /* NEW: dense-tile split limits (0: defaults) */

/* ---- NEW: multi-GPU frames (tile-row sharding + RCCL assembly) */
typedef struct NrComm NrComm;
bool GetCommUniqueId(iu8* out128);              /* rank 0: 128-byte RCCL id to distribute */
NrComm* CreateComm(i64 nranks, i64 rank, const iu8* id128); /* on the current device */
void DestroyComm(NrComm* comm);
void SetShard(RenderContext* ctx, i64 nshards, i64 shard);  /* own tile rows ty % nshards == shard */
void SetShardSlots(RenderContext* ctx, i64 nshards, i64 shard, const i64* slots); /* weighted: rank p owns slots[p]
                                                 of every sum(slots) <= 64 bands, interleaved (same call on all ranks) */
i64 GetShardPattern(RenderContext* ctx, iu8* out64);   /* band b -> rank out64[b % period]; returns the period */
bool GatherFrameU8(RenderContext* ctx, NrComm* comm, i64 root);  /* u8 frame (cpp:52-57) assembled on root */
bool GetFrameU8(RenderContext* ctx, iu8* out);
void* GetFrameU8DevicePtr(RenderContext* ctx);
i64 DeliverFrameU8(RenderContext* ctx, iu8* host);  /* async D2H of that frame into pinned `host` on the gather
                                                       stream, overlapped with the next frame; -> ticket (-1: none) */
bool WaitFrameDelivered(RenderContext* ctx, i64 ticket);
void* AllocHostBuffer(i64 bytes);                   /* pinned host memory (DeliverFrameU8 targets) */
void FreeHostBuffer(void* p);
i64 DeliverFrameBands(RenderContext* ctx, iu8* host); /* §8e: this rank's bands of its frame output straight into
                                                       their places in a host frame (every rank into the same one:
                                                       assembled by each GPU's own PCIe link, no GPU ingress);
                                                       async on the gather stream -> ticket for WaitFrameDelivered.
                                                       `host` should be pinned (AllocHostBuffer /
                                                       AllocSharedHostBuffer): small shares are then written by a
                                                       copy kernel through its device address; any other host
                                                       pointer takes the (slower) runtime copies */
void* AllocSharedHostBuffer(const char* name, i64 bytes); /* pinned POSIX shared memory "/name" (one host frame for
                                                       the processes of a sharded frame) */
void FreeSharedHostBuffer(void* p, i64 bytes);
bool UnlinkSharedHostBuffer(const char* name);
bool SetFrameFormat(RenderContext* ctx, i64 format); /* 0: u8 image (default), 1: YUV420P planes written by the
                                                       raster and gathered as such (W, H even; same on all ranks) */
i64 GetFrameFormat(RenderContext* ctx);
bool GetFrameYUV420P(RenderContext* ctx, iu8* out); /* §8f-2: YUV420P planes of that frame (W, H even), the
                                                       encoder input of PutRendererContextFrame (cpp:232-275) */
bool GatherFramebuffer(RenderContext* ctx, NrComm* comm, i64 root); /* f64 + depth bands to root (a rank without
                                                       a depth buffer sends its cleared one) */
bool GatherFramebufferEx(RenderContext* ctx, NrComm* comm, i64 root, bool withDepth); /* withDepth: the same on
                                                       every rank (it alone decides the posted send/recvs) */
bool GatherFrameU8Local(RenderContext** ctxs, i64 n, i64 root); /* tests: GatherFrameU8's packed assembly of n
                                                                    shards of one process, device copies for RCCL */
bool GatherFrameU8LocalRccl(RenderContext** ctxs, i64 n, i64 root, NrComm* self); /* tests: the same with the packs
                                              moved by RCCL send/recv pairs over a one-rank communicator `self` */

/* ---- NEW: deferred command list ---------------------------
 * Replaces the reference's recording proxy MultiThreadedVideoRenderContext-
 * Preparer (libNativeCPURendererPybind.py:302-367, whose replay is a stub).
 * While recording, DrawTexture / DrawSplittedTexture / DrawRect / DrawLine /
 * DrawCircle / DrawVerticalGrd / FillColor / ApplyPixel / SetPixel are queued
 * and then run together by ONE launch, per pixel in recording order, with the
 * exact results of the immediate calls (every pixel read and written once per
 * list instead of once per draw).  Any call that reads or otherwise touches
 * the framebuffer runs the queue first; SetColor discards it (overwritten). */
void BeginCommandList(RenderContext* ctx);       /* start queueing primitive draws */
void EndCommandList(RenderContext* ctx);         /* run the queue, stop queueing */
void FlushCommandList(RenderContext* ctx);       /* run the queue, keep queueing (end of a frame) */
i64 GetCommandListLength(RenderContext* ctx);    /* draws queued and not yet run */
bool IsRecordingCommands(RenderContext* ctx);
/* A frame's draw and state calls as ONE packed f64 array (replaces the reference's
 * per-call ctypes round trips, Pybind:74-300; its unfinished frame recorder is
 * Pybind:302-367).  Command = opcode word + fixed arguments, run in order through
 * the same entry points as the single calls (bit-identical):
 *   0 SaveContextState  1 RestoreContextState  2 SetTransform a..f  3 ApplyTransform a..f
 *   4 Scale sx sy  5 Translate tx ty  6 Rotate angle  7 SetColorTransform rgba
 *   8 ApplyColorTransform rgba  9 SetColor rgba  10 FillColor rgba
 *   11 DrawTexture tex x y w h  12 DrawSplittedTexture tex x y w h uS uE vS vE
 *   13 DrawRect x y w h rgba  14 DrawLine x1 y1 x2 y2 width rgba  15 DrawCircle x y radius rgba
 *   16 DrawVerticalGrd x y w h top-rgba bottom-rgba  17 SetPixel x y rgba  18 ApplyPixel x y rgba
 * (tex: index into `textures`).  Returns the commands run, -1 on a malformed array
 * (the commands before the bad one have run; error latched). */
i64 ExecuteCommands(RenderContext* ctx, const f64* words, i64 nwords, Texture* const* textures, i64 ntextures);

/* ---- NEW: device, sync, interop, errors, measurement --------------------- */
bool SetDevice(i64 device);                      /* device for objects created next on this thread */
i64 GetDeviceCount(void);
i64 GetContextDevice(RenderContext* ctx);
void Flush(RenderContext* ctx);                  /* wait for every queued draw */
void ResolvePending(RenderContext* ctx);         /* materialise deferred clears */
void* GetDeviceBufferPtr(RenderContext* ctx);    /* framebuffer in HBM (RCCL / interop); writes the pending
                                                    clears first -- the bytes are current after Flush */
void* GetStreamPtr(RenderContext* ctx);          /* hipStream_t the context launches on */
void GetBufferAsUInt8Device(RenderContext* ctx, iu8* dev_out); /* cpp:52-57 into HBM */
void GetTextureBuffer(Texture* tex, f64* out);
const char* GetLastErrorString(void);            /* "" when no HIP call failed */
void ClearLastError(void);
void EnableKernelTiming(RenderContext* ctx, bool on);
bool GetKernelTiming(RenderContext* ctx, const char* name, f64* total_ms, i64* count);
void ResetKernelTiming(RenderContext* ctx);
void SetKernelTimingFilter(RenderContext* ctx, const char* names); /* comma-separated kernel names, "" = all */

#ifdef __cplusplus
}
#endif
#endif
