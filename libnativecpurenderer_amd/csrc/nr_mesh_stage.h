// nr_mesh_stage.h — the layouts of a mesh draw's staging (TriScratch::mstage), in doubles.  Plain C++ with no
// HIP dependency: tests/test_mesh_stage.py compiles it with the host compiler and checks every layout.
//
// A layout is carved by a bump allocator whose every region starts at an even offset, so each region is 16-byte
// aligned -- the kernels read and write most of them as double2 -- because the carve says so, not because a call
// site padded the region in front of it.  Offsets are resolved against the buffer only after
// mstage.ensure(total) has returned: ensure may move the buffer.
#pragma once
#include <cstddef>

namespace nrmesh {

struct Carve {
    size_t used = 0;
    // The offset of a region of `count` doubles; the next one starts `count` rounded up to even behind it.
    size_t take(size_t count) {
        const size_t at = used;
        used += (count + 1) & ~(size_t)1;
        return at;
    }
    size_t total() const { return used; }   // what mstage.ensure() is asked for
};

// The regions a draw may have; count 0: the layout has no such region.
enum Region {
    R_VXY, R_VZ, R_VQ,    // the vertex table: (x, y) NV*2, z NV, and a perspective draw's 1/cw NV
    R_TABLE,              // a lit draw's vertex colours NV*4
    R_XY, R_Z, R_ATTR,    // the soup: xy T*6, z T*3, its own attributes T*stride (else the mesh's expanded ones)
    R_Q,                  // the soup's 1/w T*3
    R_EXPANDED,           // a clipped lit draw: the colour table through the indices, N*stride, the emit pass's input
    R_COUNT
};

struct Stage {
    struct Span { size_t at, count; } r[R_COUNT] = {};
    size_t total = 0;
    void take(Carve& c, Region k, size_t count) {
        r[k] = Span{c.take(count), count};
        total = c.total();
    }
    template <class T>
    T* at(T* base, Region k) const { return r[k].count ? base + r[k].at : nullptr; }
};

// What a draw is, as far as its staging goes.  NV vertices and N triangles in all (an instanced draw: K times the
// mesh's); persp: the vertex stage keeps 1/cw; lit: a light pass writes a colour table; unitQ: a textured colour
// draw without the perspective state, whose q is all 1.0; ownAttr: an unclipped soup with attributes of its own (a
// lit or an instanced draw; a clipped soup always has them), `stride` doubles a triangle.
struct StageNeeds {
    size_t NV, N;
    bool persp, lit, unitQ, ownAttr;
    size_t stride;
};

// The clip state off: vertex table | colour table | soup, T = N.
inline Stage stage_unclipped(const StageNeeds& d) {
    Stage s;
    Carve c;
    s.take(c, R_VXY, d.NV * 2);
    s.take(c, R_VZ, d.NV);
    if (d.persp) s.take(c, R_VQ, d.NV);
    if (d.lit) s.take(c, R_TABLE, d.NV * 4);
    s.take(c, R_XY, d.N * 6);
    s.take(c, R_Z, d.N * 3);
    if (d.ownAttr) s.take(c, R_ATTR, d.N * d.stride);
    if (d.persp || d.unitQ) s.take(c, R_Q, d.N * 3);
    return s;
}

// The clip state on, carved once the count nout of output triangles is known: soup (T = nout) | a lit draw's
// colour table and its expansion.  (Clip coordinates, keep masks and offsets: TriScratch::mclip and mscan.)
inline Stage stage_clipped(const StageNeeds& d, size_t nout) {
    Stage s;
    Carve c;
    s.take(c, R_XY, nout * 6);
    s.take(c, R_Z, nout * 3);
    s.take(c, R_ATTR, nout * d.stride);
    if (d.persp || d.unitQ) s.take(c, R_Q, nout * 3);
    if (d.lit) {
        s.take(c, R_TABLE, d.NV * 4);
        s.take(c, R_EXPANDED, d.N * d.stride);
    }
    return s;
}

}  // namespace nrmesh
