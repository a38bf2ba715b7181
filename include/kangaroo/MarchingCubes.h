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
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <kfx_mesh.h>
#include <kfx_mesh_index.h>

#include <kangaroo/BoundedVolume.h>
#include <kangaroo/Sdf.h>
#include <kangaroo/launch_utils.h>

namespace roo
{

namespace mesh_detail
{
inline void* DeviceBytes(size_t n)
{
    void* p = nullptr;
    size_t pitch = 0;
    GpuCheckStatus(kfx_alloc_pitched(&p, &pitch, n ? n : 1, 1));
    return p;
}

template<typename T> struct Cell;
template<> struct Cell<SDF_t> { static constexpr int kind = KFX_CELL_F32; };
template<> struct Cell<SDF_h> { static constexpr int kind = KFX_CELL_F16; };

// The mesh of `vol` (slab: its cubes [own_lo, own_hi) of the volume `slab` describes) as host arrays: 3 vertices per triangle
struct HostMesh {
    std::vector<float> v, n, c;   // x y z, nx ny nz, r g b a
    size_t ntri = 0;
    bool color = false;
};
inline HostMesh Extract(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol)
{
    HostMesh m;
    const size_t nbytes = kfx_mesh_scratch_bytes(vol, cell, slab, own_lo, own_hi);
    if (!nbytes) GpuCheckStatus(kfx_mesh_plan(vol, cell, slab, own_lo, own_hi, nullptr, 0, nullptr, 0));   // the reason
    void* scratch = DeviceBytes(nbytes);
    unsigned long long totals[2] = {0, 0};
    const int e = kfx_mesh_plan(vol, cell, slab, own_lo, own_hi, scratch, nbytes, totals, 0);
    if (e) { kfx_free(scratch); GpuCheckStatus(e); }
    const size_t na = totals[0], nv = 3 * totals[1];
    m.ntri = totals[1];
    m.color = colorvol != nullptr;
    long long* dactive = (long long*)DeviceBytes(na * 8);
    unsigned* doffsets = (unsigned*)DeviceBytes(na * 4);
    float* dv = (float*)DeviceBytes(nv * 12);
    float* dn = (float*)DeviceBytes(nv * 12);
    float* dc = m.color ? (float*)DeviceBytes(nv * 16) : nullptr;
    if (na) GpuCheckStatus(kfx_mesh_emit(vol, cell, slab, own_lo, own_hi, colorvol, scratch, nbytes, totals, dactive, doffsets, dv, dn, dc, 0));
    m.v.resize(nv * 3); m.n.resize(nv * 3); m.c.resize(m.color ? nv * 4 : 0);
    if (nv) {
        GpuCheckStatus(kfx_memcpy_2d(m.v.data(), nv * 12, dv, nv * 12, nv * 12, 1, 2, 0));
        GpuCheckStatus(kfx_memcpy_2d(m.n.data(), nv * 12, dn, nv * 12, nv * 12, 1, 2, 0));
        if (m.color) GpuCheckStatus(kfx_memcpy_2d(m.c.data(), nv * 16, dc, nv * 16, nv * 16, 1, 2, 0));
    }
    kfx_free(scratch); kfx_free(dactive); kfx_free(doffsets); kfx_free(dv); kfx_free(dn);
    if (dc) kfx_free(dc);
    return m;
}

// binary little-endian PLY; returns the triangle count, 0 if the file cannot be written
inline size_t WritePly(const std::string& path, const HostMesh& m)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return 0;
    const size_t nv = 3 * m.ntri;
    fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment kangaroo_amd marching cubes\nelement vertex %zu\n", nv);
    fprintf(f, "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n");
    if (m.color) fprintf(f, "property float red\nproperty float green\nproperty float blue\nproperty float alpha\n");
    fprintf(f, "element face %zu\nproperty list uchar uint vertex_indices\nend_header\n", m.ntri);
    for (size_t i = 0; i < nv; ++i) {
        fwrite(&m.v[i * 3], 4, 3, f);
        fwrite(&m.n[i * 3], 4, 3, f);
        if (m.color) fwrite(&m.c[i * 4], 4, 4, f);
    }
    for (size_t t = 0; t < m.ntri; ++t) {
        const unsigned char k = 3;
        const uint32_t idx[3] = {(uint32_t)(3 * t), (uint32_t)(3 * t + 1), (uint32_t)(3 * t + 2)};
        fwrite(&k, 1, 1, f);
        fwrite(idx, 4, 3, f);
    }
    fclose(f);
    return m.ntri;
}

// The indexed mesh (include/kfx_mesh_index.h): the soup above welded by lattice edge on the device -- nvert vertices in v, n, c and
// three vertex ids per triangle in faces.
struct HostIndexedMesh {
    std::vector<float> v, n, c;   // x y z, nx ny nz, r g b a
    std::vector<uint32_t> faces;
    size_t ntri = 0, nvert = 0;
    bool color = false;
};
inline HostIndexedMesh ExtractIndexed(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol)
{
    HostIndexedMesh m;
    const size_t nbytes = kfx_mesh_scratch_bytes(vol, cell, slab, own_lo, own_hi);
    if (!nbytes) GpuCheckStatus(kfx_mesh_plan(vol, cell, slab, own_lo, own_hi, nullptr, 0, nullptr, 0));   // the reason
    void* scratch = DeviceBytes(nbytes);
    unsigned long long totals[2] = {0, 0}, nvert = 0;
    int e = kfx_mesh_plan(vol, cell, slab, own_lo, own_hi, scratch, nbytes, totals, 0);
    if (e) { kfx_free(scratch); GpuCheckStatus(e); }
    const size_t xbytes = kfx_mesh_index_scratch_bytes(vol, cell, slab, own_lo, own_hi, totals);
    void* xscratch = DeviceBytes(xbytes);
    e = kfx_mesh_index_plan(vol, cell, slab, own_lo, own_hi, scratch, nbytes, totals, xscratch, xbytes, &nvert, 0);
    kfx_free(scratch);
    if (e) { kfx_free(xscratch); GpuCheckStatus(e); }
    const size_t nv = nvert, nf = 3 * totals[1];
    m.ntri = totals[1];
    m.nvert = nv;
    m.color = colorvol != nullptr;
    float* dv = (float*)DeviceBytes(nv * 12);
    float* dn = (float*)DeviceBytes(nv * 12);
    float* dc = m.color ? (float*)DeviceBytes(nv * 16) : nullptr;
    unsigned* df = (unsigned*)DeviceBytes(nf * 4);
    if (totals[0]) GpuCheckStatus(kfx_mesh_emit_indexed(vol, cell, slab, own_lo, own_hi, colorvol, xscratch, xbytes, totals, nvert, dv, dn, dc, df, 0));
    m.v.resize(nv * 3); m.n.resize(nv * 3); m.c.resize(m.color ? nv * 4 : 0); m.faces.resize(nf);
    if (nv) {
        GpuCheckStatus(kfx_memcpy_2d(m.v.data(), nv * 12, dv, nv * 12, nv * 12, 1, 2, 0));
        GpuCheckStatus(kfx_memcpy_2d(m.n.data(), nv * 12, dn, nv * 12, nv * 12, 1, 2, 0));
        if (m.color) GpuCheckStatus(kfx_memcpy_2d(m.c.data(), nv * 16, dc, nv * 16, nv * 16, 1, 2, 0));
        GpuCheckStatus(kfx_memcpy_2d(m.faces.data(), nf * 4, df, nf * 4, nf * 4, 1, 2, 0));
    }
    kfx_free(xscratch); kfx_free(dv); kfx_free(dn); kfx_free(df);
    if (dc) kfx_free(dc);
    return m;
}

// binary little-endian PLY of an indexed mesh: nvert vertex records, ntri faces; returns the triangle count, 0 if the file cannot be written
inline size_t WritePly(const std::string& path, const HostIndexedMesh& m)
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
        fwrite(&k, 1, 1, f);
        fwrite(&m.faces[t * 3], 4, 3, f);
    }
    fclose(f);
    return m.ntri;
}
}

// Returns the number of triangles written.  T = SDF_t or SDF_h (half cells: the mesh of the widened volume).
template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMesh(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>* volColor)
{
    const bool color = volColor && volColor->IsValid();
    const mesh_detail::HostMesh m = mesh_detail::Extract(vol.abi(), mesh_detail::Cell<T>::kind, nullptr, 0, 0, color ? volColor->abi() : nullptr);
    return mesh_detail::WritePly(filename + ".ply", m);
}

template<typename Manage>
inline size_t SaveMesh(std::string filename, BoundedVolume<SDF_t,TargetDevice,Manage>& vol)
{
    return SaveMesh<SDF_t,Manage,Manage>(filename, vol, nullptr);
}

template<typename Manage1, typename Manage2>
inline size_t SaveMesh(std::string filename, BoundedVolume<SDF_t,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor)
{
    return SaveMesh<SDF_t,Manage1,Manage2>(filename, vol, &volColor);
}

// half cells (BoundedVolume<SDF_h>, config C5)
template<typename Manage>
inline size_t SaveMesh(std::string filename, BoundedVolume<SDF_h,TargetDevice,Manage>& vol)
{
    return SaveMesh<SDF_h,Manage,Manage>(filename, vol, nullptr);
}

template<typename Manage1, typename Manage2>
inline size_t SaveMesh(std::string filename, BoundedVolume<SDF_h,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor)
{
    return SaveMesh<SDF_h,Manage1,Manage2>(filename, vol, &volColor);
}

// SaveMeshIndexed(filename, vol[, volColor]): SaveMesh's mesh welded by lattice edge (include/kfx_mesh_index.h) -- the first-occurrence
// vertices of SaveMesh's file and a face list in its triangle order.  Returns the number of triangles written; nvert, if given, receives
// the number of vertices.  T = SDF_t or SDF_h.
template<typename T, typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<T,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>* volColor, size_t* nvert = nullptr)
{
    const bool color = volColor && volColor->IsValid();
    const mesh_detail::HostIndexedMesh m = mesh_detail::ExtractIndexed(vol.abi(), mesh_detail::Cell<T>::kind, nullptr, 0, 0, color ? volColor->abi() : nullptr);
    if (nvert) *nvert = m.nvert;
    return mesh_detail::WritePly(filename + ".ply", m);
}

template<typename Manage>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<SDF_t,TargetDevice,Manage>& vol, size_t* nvert = nullptr)
{
    return SaveMeshIndexed<SDF_t,Manage,Manage>(filename, vol, nullptr, nvert);
}

template<typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<SDF_t,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor, size_t* nvert = nullptr)
{
    return SaveMeshIndexed<SDF_t,Manage1,Manage2>(filename, vol, &volColor, nvert);
}

template<typename Manage>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<SDF_h,TargetDevice,Manage>& vol, size_t* nvert = nullptr)
{
    return SaveMeshIndexed<SDF_h,Manage,Manage>(filename, vol, nullptr, nvert);
}

template<typename Manage1, typename Manage2>
inline size_t SaveMeshIndexed(std::string filename, BoundedVolume<SDF_h,TargetDevice,Manage1>& vol, BoundedVolume<float,TargetDevice,Manage2>& volColor, size_t* nvert = nullptr)
{
    return SaveMeshIndexed<SDF_h,Manage1,Manage2>(filename, vol, &volColor, nvert);
}

}
