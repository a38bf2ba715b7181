// MarchingCubes.h -- roo::SaveMesh (reference include/kangaroo/MarchingCubes.h:205-262): iso-surface of a device
// BoundedVolume<SDF_t> or BoundedVolume<SDF_h>, optionally coloured from a BoundedVolume<float>, written as <filename>.ply.
// The reference marches the cubes on the host after copying the volume back and exports through Assimp; here the
// extraction runs on the GPU (include/kfx_mesh.h: kfx_mesh_plan counts and scans on the device, kfx_mesh_emit compacts and
// emits) and only the finished vertex arrays are copied.  Vertex order, positions, normals and colours follow the reference's
// loop nest and expressions; half cells are meshed as the exactly widened volume (SDF_h's operator float).  The case tables
// are this repo's own derivation (scripts/gen_mc_tables.py, same boundary loops and winding as the classic tables in all 256
// cases).  PLY layout: x y z nx ny nz [red green blue alpha] floats, one face per three consecutive vertices, binary little endian.
// roo::SaveMeshIndexed (an addition; SaveMesh keeps the reference's signature and output) writes the same surface with one vertex per
// lattice edge and a face list, welded on the device (include/kfx_mesh_index.h): about a third of the bytes, usable for adjacency.
// roo::MeshComponents / roo::MeshFilter (include/kfx_mesh_clean.h) use that adjacency on the device: the connected components of an
// indexed mesh, and the mesh without its small ones -- the floaters around the surface; SaveMeshIndexed takes min_faces / largest.
// roo::MeshSimplify (include/kfx_mesh_simplify.h) is the level of detail after them: the vertices of one cell of a world-anchored grid
// become one, on the device; SaveMeshIndexed(..., min_faces, largest, nvert, cell) applies it after the filter.
// roo::MeshAdjacency / roo::MeshSmooth / roo::MeshVertexNormals (include/kfx_mesh_smooth.h) come last: every vertex's face corners in
// ascending order, Laplacian / Taubin passes that sum in that order, and normals recomputed from the faces;
// SaveMeshIndexed(..., min_faces, largest, nvert, cell, smooth_iterations) applies them after the other two.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <kfx_mesh.h>
#include <kfx_mesh_index.h>
#include <kfx_mesh_clean.h>
#include <kfx_mesh_simplify.h>
#include <kfx_mesh_smooth.h>

#include <kangaroo/BoundedVolume.h>
#include <kangaroo/Sdf.h>
#include <kangaroo/launch_utils.h>

namespace roo
{

namespace mesh_detail
{
// n bytes of device memory (at least one), freed with the object; move-only
class DeviceBuffer
{
public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t n)
    {
        size_t pitch = 0;
        GpuCheckStatus(kfx_alloc_pitched(&ptr_, &pitch, n ? n : 1, 1));
    }
    DeviceBuffer(DeviceBuffer&& o) noexcept : ptr_(o.ptr_) { o.ptr_ = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) { Free(); ptr_ = o.ptr_; o.ptr_ = nullptr; }
        return *this;
    }
    ~DeviceBuffer() { Free(); }
    template<typename T = void> T* get() const { return (T*)ptr_; }
    // its first n bytes into host memory
    void CopyTo(void* host, size_t n) const
    {
        if (n) GpuCheckStatus(kfx_memcpy_2d(host, n, ptr_, n, n, 1, 2, 0));
    }
private:
    void Free() { if (ptr_) kfx_free(ptr_); ptr_ = nullptr; }
    void* ptr_ = nullptr;
};

template<typename T> struct Cell;
template<> struct Cell<SDF_t> { static constexpr int kind = KFX_CELL_F32; };
template<> struct Cell<SDF_h> { static constexpr int kind = KFX_CELL_F16; };

// A mesh as host arrays.  The soup: three vertices per triangle, nvert = 3 ntri, faces empty (triangle t is vertices 3t, 3t + 1, 3t + 2).
// The indexed mesh (include/kfx_mesh_index.h): the soup welded by lattice edge on the device, three vertex ids per triangle in faces.
struct HostMesh {
    std::vector<float> v, n, c;   // x y z, nx ny nz, r g b a
    std::vector<uint32_t> faces;
    size_t ntri = 0, nvert = 0;
    bool color = false;
};

// What a clean-up keeps (include/kfx_mesh_clean.h): the components with at least min_faces faces; largest: only the one with the most.
struct MeshKeep {
    size_t min_faces = 0;
    bool largest = false;
    explicit operator bool() const { return min_faces || largest; }
};

// An indexed mesh in device memory -- nv rows of dv, dn and (where dc holds any) dc, nt rows of faces -- replaced by what `keep` keeps
// of it: kfx_mesh_components_plan, kfx_mesh_filter_plan, kfx_mesh_filter_emit.
inline void FilterBuffers(DeviceBuffer& dv, DeviceBuffer& dn, DeviceBuffer& dc, DeviceBuffer& faces, size_t& nv, size_t& nt, const MeshKeep& keep)
{
    const size_t nbytes = kfx_mesh_components_scratch_bytes(nv, nt);
    DeviceBuffer scratch(nbytes);
    unsigned long long counts[2] = {0, 0}, kept[2] = {0, 0};
    GpuCheckStatus(kfx_mesh_components_plan(faces.get<unsigned>(), nt, nv, scratch.get(), nbytes, counts, 0));   // (nbytes 0: the reason)
    GpuCheckStatus(kfx_mesh_filter_plan(scratch.get(), nbytes, nv, nt, faces.get<unsigned>(), keep.min_faces, keep.largest, kept, 0));
    DeviceBuffer ov(kept[0] * 12), on, oc, of(kept[1] * 12);
    if (dn.get()) on = DeviceBuffer(kept[0] * 12);
    if (dc.get()) oc = DeviceBuffer(kept[0] * 16);
    GpuCheckStatus(kfx_mesh_filter_emit(scratch.get(), nbytes, nv, nt, kept, dv.get<float>(), dn.get<float>(), dc.get<float>(), faces.get<unsigned>(),
                                        ov.get<float>(), on.get<float>(), oc.get<float>(), of.get<unsigned>(), 0));
    dv = std::move(ov); dn = std::move(on); dc = std::move(oc); faces = std::move(of);
    nv = kept[0];
    nt = kept[1];
}

// An indexed mesh in device memory replaced by its simplification on a grid of `cell` world units anchored at the world origin
// (include/kfx_mesh_simplify.h): kfx_mesh_simplify_plan, kfx_mesh_simplify_emit.
inline void SimplifyBuffers(DeviceBuffer& dv, DeviceBuffer& dn, DeviceBuffer& dc, DeviceBuffer& faces, size_t& nv, size_t& nt, float cell)
{
    const size_t nbytes = kfx_mesh_simplify_scratch_bytes(nv, nt);
    DeviceBuffer scratch(nbytes);
    const float origin[3] = {0.0f, 0.0f, 0.0f};
    unsigned long long kept[2] = {0, 0};
    GpuCheckStatus(kfx_mesh_simplify_plan(dv.get<float>(), faces.get<unsigned>(), nt, nv, origin, cell, scratch.get(), nbytes, kept, 0));   // (nbytes 0: the reason)
    DeviceBuffer ov(kept[0] * 12), on, oc, of(kept[1] * 12);
    if (dn.get()) on = DeviceBuffer(kept[0] * 12);
    if (dc.get()) oc = DeviceBuffer(kept[0] * 16);
    GpuCheckStatus(kfx_mesh_simplify_emit(scratch.get(), nbytes, nv, nt, kept, dv.get<float>(), dn.get<float>(), dc.get<float>(), faces.get<unsigned>(),
                                          ov.get<float>(), on.get<float>(), oc.get<float>(), of.get<unsigned>(), nullptr, 0));
    dv = std::move(ov); dn = std::move(on); dc = std::move(oc); faces = std::move(of);
    nv = kept[0];
    nt = kept[1];
}

// The parameters of a smoothing (include/kfx_mesh_smooth.h): Taubin's by default, the open boundary pinned
struct MeshSmoothing {
    int iterations = 5;
    float lambda = 0.5f, mu = -0.53f;
    bool pin_boundary = true;
};

// The incidence lists of nt faces over nv vertices in device memory: start (nv + 1 words), inc (3 nt words) and, if asked for, flags (nv words)
struct DeviceAdjacency {
    DeviceBuffer start, inc, flags;
};
inline DeviceAdjacency Adjacency(const unsigned* faces, size_t nv, size_t nt, bool with_flags)
{
    DeviceAdjacency a;
    const size_t nbytes = kfx_mesh_adjacency_scratch_bytes(nv, nt);
    DeviceBuffer scratch(nbytes);
    a.start = DeviceBuffer((nv + 1) * 4);
    a.inc = DeviceBuffer(nt * 12);
    if (with_flags) a.flags = DeviceBuffer(nv * 4);
    GpuCheckStatus(kfx_mesh_adjacency(faces, nt, nv, a.start.get<unsigned>(), a.inc.get<unsigned>(), a.flags.get<unsigned>(), scratch.get(), nbytes, 0));   // (nbytes 0: the reason)
    return a;
}

// nv vertices in device memory after a smoothing, in a new buffer; and their normals from the faces
inline DeviceBuffer SmoothedVertices(const float* verts, const unsigned* faces, size_t nv, size_t nt, const DeviceAdjacency& a, const MeshSmoothing& how)
{
    const size_t nbytes = kfx_mesh_smooth_scratch_bytes(nv, nt);
    DeviceBuffer scratch(nbytes), out(nv * 12);
    GpuCheckStatus(kfx_mesh_smooth(verts, faces, nt, nv, a.start.get<unsigned>(), a.inc.get<unsigned>(), how.pin_boundary ? a.flags.get<unsigned>() : nullptr,
                                   how.iterations, how.lambda, how.mu, how.pin_boundary ? KFX_MESH_BOUNDARY : 0u, out.get<float>(), scratch.get(), nbytes, 0));
    return out;
}
inline DeviceBuffer Normals(const float* verts, const unsigned* faces, size_t nv, size_t nt, const DeviceAdjacency& a)
{
    DeviceBuffer scratch(256), out(nv * 12);
    GpuCheckStatus(kfx_mesh_vertex_normals(verts, faces, nt, nv, a.start.get<unsigned>(), a.inc.get<unsigned>(), out.get<float>(), scratch.get(), 256, 0));
    return out;
}

// An indexed mesh in device memory with its vertices smoothed and its normals (where it has any) recomputed from the faces; colours and
// faces stay as they are
inline void SmoothBuffers(DeviceBuffer& dv, DeviceBuffer& dn, const DeviceBuffer& faces, size_t nv, size_t nt, const MeshSmoothing& how)
{
    const DeviceAdjacency a = Adjacency(faces.get<unsigned>(), nv, nt, how.pin_boundary);
    dv = SmoothedVertices(dv.get<float>(), faces.get<unsigned>(), nv, nt, a, how);
    if (dn.get()) dn = Normals(dv.get<float>(), faces.get<unsigned>(), nv, nt, a);
}

// The mesh of `vol` (slab: its cubes [own_lo, own_hi) of the volume `slab` describes); keep: an indexed mesh without its small components;
// simplify_cell > 0: then simplified on a grid of that cell (0: off); smooth_iterations > 0: then smoothed, MeshSmoothing's defaults (0: off)
inline HostMesh Extract(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol, bool indexed = false,
                        const MeshKeep& keep = MeshKeep(), float simplify_cell = 0.0f, int smooth_iterations = 0)
{
    const size_t nbytes = kfx_mesh_scratch_bytes(vol, cell, slab, own_lo, own_hi);
    if (!nbytes) GpuCheckStatus(kfx_mesh_plan(vol, cell, slab, own_lo, own_hi, nullptr, 0, nullptr, 0));   // the reason
    DeviceBuffer scratch(nbytes), xscratch, active, offsets, faces;
    unsigned long long totals[2] = {0, 0}, nvert = 0;
    GpuCheckStatus(kfx_mesh_plan(vol, cell, slab, own_lo, own_hi, scratch.get(), nbytes, totals, 0));
    HostMesh m;
    m.ntri = totals[1];
    m.nvert = 3 * m.ntri;
    m.color = colorvol != nullptr;
    size_t xbytes = 0;
    if (indexed) {
        xbytes = kfx_mesh_index_scratch_bytes(vol, cell, slab, own_lo, own_hi, totals);
        xscratch = DeviceBuffer(xbytes);
        GpuCheckStatus(kfx_mesh_index_plan(vol, cell, slab, own_lo, own_hi, scratch.get(), nbytes, totals, xscratch.get(), xbytes, &nvert, 0));
        scratch = DeviceBuffer();   // (the indexed emit reads the index scratch alone)
        m.nvert = nvert;
        m.faces.resize(3 * m.ntri);
        faces = DeviceBuffer(m.faces.size() * 4);
    } else {
        active = DeviceBuffer(totals[0] * 8);
        offsets = DeviceBuffer(totals[0] * 4);
    }
    size_t nv = m.nvert;
    DeviceBuffer dv(nv * 12), dn(nv * 12), dc;
    if (m.color) dc = DeviceBuffer(nv * 16);
    if (totals[0] && indexed)
        GpuCheckStatus(kfx_mesh_emit_indexed(vol, cell, slab, own_lo, own_hi, colorvol, xscratch.get(), xbytes, totals, nvert, dv.get<float>(),
                                             dn.get<float>(), dc.get<float>(), faces.get<unsigned>(), 0));
    else if (totals[0])
        GpuCheckStatus(kfx_mesh_emit(vol, cell, slab, own_lo, own_hi, colorvol, scratch.get(), nbytes, totals, active.get<long long>(),
                                     offsets.get<unsigned>(), dv.get<float>(), dn.get<float>(), dc.get<float>(), 0));
    if (keep && indexed && m.ntri) {
        FilterBuffers(dv, dn, dc, faces, nv, m.ntri, keep);
        m.nvert = nv;
        m.faces.resize(3 * m.ntri);
    }
    if (simplify_cell != 0.0f && indexed && m.ntri) {   // (floaters go first: clustering changes face counts)
        SimplifyBuffers(dv, dn, dc, faces, nv, m.ntri, simplify_cell);
        m.nvert = nv;
        m.faces.resize(3 * m.ntri);
    }
    if (smooth_iterations != 0 && indexed && m.ntri) {   // (last: it moves what the other two copy)
        MeshSmoothing how;
        how.iterations = smooth_iterations;
        SmoothBuffers(dv, dn, faces, nv, m.ntri, how);
    }
    m.v.resize(nv * 3); m.n.resize(nv * 3); m.c.resize(m.color ? nv * 4 : 0);
    dv.CopyTo(m.v.data(), nv * 12);
    dn.CopyTo(m.n.data(), nv * 12);
    dc.CopyTo(m.c.data(), m.c.size() * 4);
    faces.CopyTo(m.faces.data(), m.faces.size() * 4);
    return m;
}

// binary little-endian PLY: nvert vertex records, ntri faces; returns the triangle count, 0 if the file cannot be written
inline size_t WritePly(const std::string& path, const HostMesh& m)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return 0;
    fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment kangaroo_amd marching cubes\nelement vertex %zu\n", m.nvert);
    fprintf(f, "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n");
    if (m.color) fprintf(f, "property float red\nproperty float green\nproperty float blue\nproperty float alpha\n");
    fprintf(f, "element face %zu\nproperty list uchar uint vertex_indices\nend_header\n", m.ntri);
    for (size_t i = 0; i < m.nvert; ++i) {
        fwrite(&m.v[i * 3], 4, 3, f);
        fwrite(&m.n[i * 3], 4, 3, f);
        if (m.color) fwrite(&m.c[i * 4], 4, 4, f);
    }
    for (size_t t = 0; t < m.ntri; ++t) {
        const unsigned char k = 3;
        const uint32_t soup[3] = {(uint32_t)(3 * t), (uint32_t)(3 * t + 1), (uint32_t)(3 * t + 2)};
        fwrite(&k, 1, 1, f);
        fwrite(m.faces.empty() ? soup : &m.faces[t * 3], 4, 3, f);
    }
    fclose(f);
    return m.ntri;
}

// SaveMesh / SaveMeshIndexed of a BoundedVolume<T>; a T without a Cell<T> does not compile
template<typename T, typename Manage1, typename Manage2>
inline size_t Save(const std::string& filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>* volColor, bool indexed, size_t* nvert,
                   const MeshKeep& keep = MeshKeep(), float simplify_cell = 0.0f, int smooth_iterations = 0)
{
    const bool color = volColor && volColor->IsValid();
    const HostMesh m = Extract(vol.abi(), Cell<T>::kind, nullptr, 0, 0, color ? volColor->abi() : nullptr, indexed, keep, simplify_cell, smooth_iterations);
    if (nvert) *nvert = m.nvert;
    return WritePly(filename + ".ply", m);
}
}

// SaveMesh(filename, vol[, volColor]): returns the number of triangles written.  T = SDF_t or SDF_h (half cells, config C5: the mesh
// of the widened volume).
template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMesh(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>* volColor)
{
    return mesh_detail::Save(filename, vol, volColor, false, nullptr);
}

template<typename T, typename Manage>
inline size_t SaveMesh(std::string filename, BoundedVolume<T,TargetDevice,Manage>& vol)
{
    return SaveMesh<T,Manage,Manage>(filename, vol, nullptr);
}

template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMesh(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor)
{
    return SaveMesh<T,Manage1,Manage2>(filename, vol, &volColor);
}

// SaveMeshIndexed(filename, vol[, volColor]): SaveMesh's mesh welded by lattice edge (include/kfx_mesh_index.h) -- the first-occurrence
// vertices of SaveMesh's file and a face list in its triangle order.  Returns the number of triangles written; nvert, if given, receives
// the number of vertices.  T = SDF_t or SDF_h.
template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>* volColor, size_t* nvert = nullptr)
{
    return mesh_detail::Save(filename, vol, volColor, true, nvert);
}

template<typename T, typename Manage>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage>& vol, size_t* nvert = nullptr)
{
    return SaveMeshIndexed<T,Manage,Manage>(filename, vol, nullptr, nvert);
}

template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor, size_t* nvert = nullptr)
{
    return SaveMeshIndexed<T,Manage1,Manage2>(filename, vol, &volColor, nvert);
}

// SaveMeshIndexed(filename, vol[, volColor], min_faces, largest): the indexed mesh without its small components, filtered on the device
// (include/kfx_mesh_clean.h) -- the components with at least min_faces faces; largest: only the one with the most, min_faces on top.
// cell > 0: what is left is then simplified on the device on a grid of `cell` world units anchored at the world origin
// (include/kfx_mesh_simplify.h); 0 means off, and min_faces = 0, largest = false filters nothing.
// smooth_iterations > 0: what is left is then smoothed on the device by that many Taubin iterations (lambda 0.5, mu -0.53, the open
// boundary pinned) and the normals are recomputed from the faces (include/kfx_mesh_smooth.h); 0 means off.
template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>* volColor, size_t min_faces,
                              bool largest, size_t* nvert = nullptr, float cell = 0.0f, int smooth_iterations = 0)
{
    return mesh_detail::Save(filename, vol, volColor, true, nvert, mesh_detail::MeshKeep{min_faces, largest}, cell, smooth_iterations);
}

template<typename T, typename Manage>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage>& vol, size_t min_faces, bool largest, size_t* nvert = nullptr, float cell = 0.0f,
                              int smooth_iterations = 0)
{
    return SaveMeshIndexed<T,Manage,Manage>(filename, vol, nullptr, min_faces, largest, nvert, cell, smooth_iterations);
}

template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor, size_t min_faces,
                              bool largest, size_t* nvert = nullptr, float cell = 0.0f, int smooth_iterations = 0)
{
    return SaveMeshIndexed<T,Manage1,Manage2>(filename, vol, &volColor, min_faces, largest, nvert, cell, smooth_iterations);
}

// MeshComponents(faces, n_faces, n_verts, vertex_component, component_faces): the connected components of an indexed mesh whose faces
// (n_faces x 3 ids < n_verts) are in device memory, labelled on the device (include/kfx_mesh_clean.h).  The host vectors receive every
// vertex's component and every component's face count; components are numbered by their smallest vertex id.  Returns their number.
inline size_t MeshComponents(const uint32_t* faces, size_t n_faces, size_t n_verts, std::vector<uint32_t>& vertex_component, std::vector<uint32_t>& component_faces)
{
    const size_t nbytes = kfx_mesh_components_scratch_bytes(n_verts, n_faces);
    mesh_detail::DeviceBuffer scratch(nbytes);
    unsigned long long counts[2] = {0, 0};
    GpuCheckStatus(kfx_mesh_components_plan(faces, n_faces, n_verts, scratch.get(), nbytes, counts, 0));   // (nbytes 0: the reason)
    vertex_component.resize(n_verts);
    component_faces.resize(counts[0]);
    mesh_detail::DeviceBuffer vc(n_verts * 4), cf(counts[0] * 4);
    GpuCheckStatus(kfx_mesh_components_emit(scratch.get(), nbytes, n_verts, n_faces, counts, vc.get<unsigned>(), cf.get<unsigned>(), 0));
    vc.CopyTo(vertex_component.data(), n_verts * 4);
    cf.CopyTo(component_faces.data(), counts[0] * 4);
    return counts[0];
}

// MeshFilter(verts, norms, colors, faces, n_verts, n_faces, min_faces, largest): an indexed mesh in device memory (norms and colors may be
// null) without its small components, as host arrays: kept vertices and faces in their order, rows bit for bit, ids renumbered.
inline mesh_detail::HostMesh MeshFilter(const float* verts, const float* norms, const float* colors, const uint32_t* faces, size_t n_verts, size_t n_faces,
                                        size_t min_faces, bool largest)
{
    const size_t nbytes = kfx_mesh_components_scratch_bytes(n_verts, n_faces);
    mesh_detail::DeviceBuffer scratch(nbytes);
    unsigned long long counts[2] = {0, 0}, kept[2] = {0, 0};
    GpuCheckStatus(kfx_mesh_components_plan(faces, n_faces, n_verts, scratch.get(), nbytes, counts, 0));
    GpuCheckStatus(kfx_mesh_filter_plan(scratch.get(), nbytes, n_verts, n_faces, faces, min_faces, largest, kept, 0));
    mesh_detail::HostMesh m;
    m.nvert = kept[0];
    m.ntri = kept[1];
    m.color = colors != nullptr;
    mesh_detail::DeviceBuffer ov(kept[0] * 12), on(norms ? kept[0] * 12 : 0), oc(colors ? kept[0] * 16 : 0), of(kept[1] * 12);
    GpuCheckStatus(kfx_mesh_filter_emit(scratch.get(), nbytes, n_verts, n_faces, kept, verts, norms, colors, faces, ov.get<float>(),
                                        norms ? on.get<float>() : nullptr, colors ? oc.get<float>() : nullptr, of.get<unsigned>(), 0));
    m.v.resize(m.nvert * 3); m.n.resize(norms ? m.nvert * 3 : 0); m.c.resize(colors ? m.nvert * 4 : 0); m.faces.resize(m.ntri * 3);
    ov.CopyTo(m.v.data(), m.v.size() * 4);
    on.CopyTo(m.n.data(), m.n.size() * 4);
    oc.CopyTo(m.c.data(), m.c.size() * 4);
    of.CopyTo(m.faces.data(), m.faces.size() * 4);
    return m;
}

// MeshSimplify(verts, norms, colors, faces, n_verts, n_faces, cell, origin[, vertex_cluster]): an indexed mesh in device memory (norms and
// colors may be null) at the level of detail of a grid of `cell` world units anchored at `origin` (null: the world origin), as host
// arrays (include/kfx_mesh_simplify.h): one vertex a cell -- the one nearest its centre, its row bit for bit --, the faces that collapse
// or repeat dropped.  vertex_cluster, if given, receives every input vertex's new id (0xffffffff: its cluster is not written).
inline mesh_detail::HostMesh MeshSimplify(const float* verts, const float* norms, const float* colors, const uint32_t* faces, size_t n_verts, size_t n_faces,
                                          float cell, const float* origin = nullptr, std::vector<uint32_t>* vertex_cluster = nullptr)
{
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const size_t nbytes = kfx_mesh_simplify_scratch_bytes(n_verts, n_faces);
    mesh_detail::DeviceBuffer scratch(nbytes);
    unsigned long long kept[2] = {0, 0};
    GpuCheckStatus(kfx_mesh_simplify_plan(verts, faces, n_faces, n_verts, origin ? origin : zero, cell, scratch.get(), nbytes, kept, 0));   // (nbytes 0: the reason)
    mesh_detail::HostMesh m;
    m.nvert = kept[0];
    m.ntri = kept[1];
    m.color = colors != nullptr;
    mesh_detail::DeviceBuffer ov(kept[0] * 12), on(norms ? kept[0] * 12 : 0), oc(colors ? kept[0] * 16 : 0), of(kept[1] * 12), map(vertex_cluster ? n_verts * 4 : 0);
    GpuCheckStatus(kfx_mesh_simplify_emit(scratch.get(), nbytes, n_verts, n_faces, kept, verts, norms, colors, faces, ov.get<float>(),
                                          norms ? on.get<float>() : nullptr, colors ? oc.get<float>() : nullptr, of.get<unsigned>(),
                                          vertex_cluster ? map.get<unsigned>() : nullptr, 0));
    m.v.resize(m.nvert * 3); m.n.resize(norms ? m.nvert * 3 : 0); m.c.resize(colors ? m.nvert * 4 : 0); m.faces.resize(m.ntri * 3);
    ov.CopyTo(m.v.data(), m.v.size() * 4);
    on.CopyTo(m.n.data(), m.n.size() * 4);
    oc.CopyTo(m.c.data(), m.c.size() * 4);
    of.CopyTo(m.faces.data(), m.faces.size() * 4);
    if (vertex_cluster) {
        vertex_cluster->resize(n_verts);
        map.CopyTo(vertex_cluster->data(), n_verts * 4);
    }
    return m;
}

// MeshAdjacency(faces, n_faces, n_verts, inc_start, inc[, vertex_flags]): the incidence lists of an indexed mesh whose faces are in device
// memory, built on the device (include/kfx_mesh_smooth.h).  The host vectors receive inc_start (n_verts + 1), inc (3 n_faces: every vertex's
// corner slots 3 f + c, ascending) and, if given, the flags KFX_MESH_BOUNDARY / NONMANIFOLD / DEGENERATE / ISOLATED of every vertex.
inline void MeshAdjacency(const uint32_t* faces, size_t n_faces, size_t n_verts, std::vector<uint32_t>& inc_start, std::vector<uint32_t>& inc,
                          std::vector<uint32_t>* vertex_flags = nullptr)
{
    const mesh_detail::DeviceAdjacency a = mesh_detail::Adjacency(faces, n_verts, n_faces, vertex_flags != nullptr);
    inc_start.assign(n_verts + 1, 0);
    inc.resize(3 * n_faces);
    if (n_faces) a.start.CopyTo(inc_start.data(), inc_start.size() * 4);
    a.inc.CopyTo(inc.data(), inc.size() * 4);
    if (vertex_flags) {
        vertex_flags->resize(n_verts);
        a.flags.CopyTo(vertex_flags->data(), n_verts * 4);
    }
}

// MeshSmooth(verts, faces, n_verts, n_faces[, how, normals]): the vertices of an indexed mesh in device memory after how.iterations
// smoothing iterations (include/kfx_mesh_smooth.h), as a host array of 3 n_verts floats; normals, if given, receives the normals of the
// smoothed mesh, recomputed from the faces.
inline std::vector<float> MeshSmooth(const float* verts, const uint32_t* faces, size_t n_verts, size_t n_faces,
                                     const mesh_detail::MeshSmoothing& how = mesh_detail::MeshSmoothing(), std::vector<float>* normals = nullptr)
{
    std::vector<float> out(3 * n_verts);
    if (!n_faces) return out;
    const mesh_detail::DeviceAdjacency a = mesh_detail::Adjacency(faces, n_verts, n_faces, how.pin_boundary);
    const mesh_detail::DeviceBuffer moved = mesh_detail::SmoothedVertices(verts, faces, n_verts, n_faces, a, how);
    moved.CopyTo(out.data(), out.size() * 4);
    if (normals) {
        normals->resize(3 * n_verts);
        mesh_detail::Normals(moved.get<float>(), faces, n_verts, n_faces, a).CopyTo(normals->data(), normals->size() * 4);
    }
    return out;
}

// MeshVertexNormals(verts, faces, n_verts, n_faces): per-vertex normals of an indexed mesh in device memory from its faces, on the side the
// extraction's normals lie on (include/kfx_mesh_smooth.h), as a host array of 3 n_verts floats; zero for a vertex in no face.
inline std::vector<float> MeshVertexNormals(const float* verts, const uint32_t* faces, size_t n_verts, size_t n_faces)
{
    std::vector<float> out(3 * n_verts, 0.0f);
    if (!n_faces) return out;
    const mesh_detail::DeviceAdjacency a = mesh_detail::Adjacency(faces, n_verts, n_faces, false);
    mesh_detail::Normals(verts, faces, n_verts, n_faces, a).CopyTo(out.data(), out.size() * 4);
    return out;
}

}
