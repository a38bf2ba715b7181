// SlabVolume.h -- a BoundedVolume<SDF_t> spread over the ranks of a node in Z-slabs, for C++ hosts (one rank per GPU, or
// one rank per host thread with the in-process transport).  Addition beside the reference API (the reference is
// single-GPU): thin wrappers over include/kfx_slab.h in the style of the roo:: operators -- same container types, same
// error convention.  Include it explicitly; <kangaroo/kangaroo.h> stays the reference's surface.
//
//   kfx_comm comm;  kfx_comm_create_rccl(&comm, rank, world, "/tmp/kfx.id", 60);        // or kfx_comm_create_threads
//   roo::SlabVolume slab(512, 512, 512, bbox, &comm);                                    // allocates this rank's planes
//   roo::SdfReset(slab.local, NaN);
//   per frame:  slab.Fuse(depth, normals, T_cw, K, trunc, max_w, mincostheta);           // + halo exchange
//               slab.Raycast(d, n, i, T_wc, K, near, far, trunc);                        // identical images on every rank
//   at the end: slab.SaveMesh("mesh.r" + std::to_string(rank));                         // this rank's part of the mesh
// Colour mode (the reference application's fuse_color, include/kfx_slab_color.h): slab.EnableColor() allocates this rank's planes of the
// colour volume beside `local` (same planes, same box; reset to 0.5); the colour overload of Fuse integrates both, Raycast then renders
// the colour volume into img, and SaveMesh writes colours -- all bit-identical to the single-volume colour operators.
#pragma once

#include <memory>
#include <stdexcept>

#include <kfx_slab.h>
#include <kfx_slab_color.h>

#include <kangaroo/BoundedVolume.h>
#include <kangaroo/Image.h>
#include <kangaroo/ImageIntrinsics.h>
#include <kangaroo/MarchingCubes.h>
#include <kangaroo/Mat.h>
#include <kangaroo/Sdf.h>
#include <kangaroo/cu_raycast.h>
#include <kangaroo/launch_utils.h>

namespace roo
{

class SlabVolume
{
public:
    enum HaloMode { HaloExchange, HaloRecompute };   // ghost planes: from the neighbours (RCCL send / recv) or integrated redundantly
    // nearest hit of per-slab marches; the march state handed from slab to slab (neighbour exchanges, one synchronisation per
    // frame); the same march with an all-reduce and a host check per round (the cross-check of the hand-over)
    enum RaycastMode { Composite, Exact, ExactAllReduce };
    // Composite: image strips sent to their owners and back (all-to-all + all-gather over the xGMI mesh), or two all-reduces
    enum MergeMode { MergeDirect, MergeAllReduce };

    kfx_slab_layout layout;
    BoundedVolume<SDF_t, TargetDevice, Manage> local; // planes [layout.s0, layout.s1) of the whole volume
    std::unique_ptr<BoundedVolume<float, TargetDevice, Manage> > color;   // the same planes of the colour volume (EnableColor), else null
    BoundingBox full_bbox;
    kfx_comm* comm;
    HaloMode halo;
    RaycastMode raycast;
    MergeMode merge;
    int tiles;        // Exact: 0 = whole-image stages (kfx_slab_raycast_exact); >= 1 = the hand-over pipelined over this many image row-tiles
    int last_rounds;

    SlabVolume(size_t w, size_t h, size_t d, const BoundingBox& bbox, kfx_comm* comm_, HaloMode halo_ = HaloExchange,
               RaycastMode raycast_ = Composite, int ghost = 2)
        : layout(MakeLayout(d, bbox, comm_, ghost)),
          local(w, h, layout.s1 - layout.s0, BoundingBox(make_float3(bbox.Min().x, bbox.Min().y, layout.local_zmin),
                                                           make_float3(bbox.Max().x, bbox.Max().y, layout.local_zmax))),
          full_bbox(bbox), comm(comm_), halo(halo_), raycast(raycast_), merge(MergeDirect), tiles(0), last_rounds(0), key_(0), payload_(0), state_(0), scratch_(0),
          strips_(0), tiled_(0), cap_(0), strips_cap_(0), tiled_cap_(0)
    {
    }
    ~SlabVolume()
    {
        kfx_free(key_); kfx_free(payload_); kfx_free(state_); kfx_free(scratch_); kfx_free(strips_); kfx_free(tiled_);
    }
    SlabVolume(const SlabVolume&) = delete;
    SlabVolume& operator=(const SlabVolume&) = delete;

    // the colour slab beside the SDF slab: the dimensions and the box of `local`, SdfReset(colorVol) = 0.5
    void EnableColor()
    {
        if (color) return;
        color.reset(new BoundedVolume<float, TargetDevice, Manage>(local.w, local.h, local.d, local.bbox));
        GpuCheckStatus(kfx_color_reset(color->abi(), 0));
    }
    bool HasColor() const { return (bool)color; }

    // SdfFuse of this rank's planes, evaluated with the whole volume's voxel positions and over the whole volume's
    // extents (bit-identical to the same planes of a single-GPU volume), then the ghost planes are brought up to date
    void Fuse(Image<float> depth, Image<float4> norm, Mat<float,3,4> T_cw, ImageIntrinsics K, float trunc_dist, float maxw, float mincostheta)
    {
        const bool own_only = halo == HaloExchange && layout.world > 1;
        const size_t first = own_only ? layout.z0 : layout.s0, count = own_only ? layout.z1 - layout.z0 : layout.s1 - layout.s0;
        kfx_volume v = *local.abi();
        v.ptr = (unsigned char*)v.ptr + (first - layout.s0) * v.img_pitch;
        v.d = count;
        const kfx_slab s = {layout.full_d, first, layout.full_zmin, layout.full_zmax};
        GpuCheckStatus(kfx_sdf_fuse_slab(&v, &s, depth.abi(), norm.abi(), T_cw.m, &K.fu, trunc_dist, maxw, mincostheta, KFX_FUSE_SLAB_EXTENT, 0));
        if (own_only) GpuCheckStatus(kfx_slab_exchange_halos(local.abi(), &layout, comm, 0));
    }

    // ... and the colour SdfFuse (SdfFuse(vol, colorVol, ...), cu_sdffusion.h) on the two slabs; with HaloExchange the colour volume's
    // ghost planes follow the SDF volume's (the same order on every rank).  Needs EnableColor().
    void Fuse(Image<float> depth, Image<float4> norm, Mat<float,3,4> T_cw, ImageIntrinsics K, Image<uchar3> img, Mat<float,3,4> T_iw,
              ImageIntrinsics Kimg, float trunc_dist, float maxw, float mincostheta)
    {
        EnableColor();
        const bool own_only = halo == HaloExchange && layout.world > 1;
        const size_t first = own_only ? layout.z0 : layout.s0, count = own_only ? layout.z1 - layout.z0 : layout.s1 - layout.s0;
        kfx_volume v = *local.abi(), c = *color->abi();
        v.ptr = (unsigned char*)v.ptr + (first - layout.s0) * v.img_pitch;
        c.ptr = (unsigned char*)c.ptr + (first - layout.s0) * c.img_pitch;
        v.d = c.d = count;
        const kfx_slab s = {layout.full_d, first, layout.full_zmin, layout.full_zmax};
        GpuCheckStatus(kfx_sdf_fuse_color_slab(&v, &c, &s, depth.abi(), norm.abi(), T_cw.m, &K.fu, img.abi(), T_iw.m, &Kimg.fu, trunc_dist, maxw, mincostheta,
                                               KFX_FUSE_SLAB_EXTENT, 0));
        if (own_only) {
            GpuCheckStatus(kfx_slab_exchange_halos(local.abi(), &layout, comm, 0));
            GpuCheckStatus(kfx_slab_exchange_halos(color->abi(), &layout, comm, 0));
        }
    }

    // Input distribution (the alternative to every rank preprocessing the frame itself): rank `root` holds the filtered depth
    // and the normal map, afterwards every rank does
    void BroadcastInputs(Image<float> depth, Image<float4> norm, int root = 0)
    {
        Reserve(depth.w * depth.h);
        GpuCheckStatus(kfx_slab_broadcast_inputs(depth.abi(), norm.abi(), payload_, root, comm, 0));   // payload_: 20 B per pixel
    }

    // RaycastSdf of the whole model; every rank returns with the same images.  With a colour slab (EnableColor) img is the colour
    // rendering, RaycastSdf(depth, norm, img, vol, colorVol, ...): Composite renders each local view in colour and merges as ever; Exact
    // hands the march over in row-tiles (one tile where `tiles` is 0: the whole-image stages have no colour form), and so does
    // ExactAllReduce (the grey hand-over's cross-check has none either).
    void Raycast(Image<float> depth, Image<float4> norm, Image<float> img, Mat<float,3,4> T_wc, ImageIntrinsics K, float near, float far,
                 float trunc_dist, bool subpix = true)
    {
        Reserve(depth.w * depth.h);
        const int tiles = (color && raycast != Composite && this->tiles < 1) ? 1 : this->tiles;
        if (color && raycast != Composite) {
            const size_t need = kfx_slab_exact_tiled_scratch_bytes(depth.w, depth.h, tiles, comm->world);
            if (need > tiled_cap_) {
                size_t pitch;
                kfx_free(tiled_);
                tiled_ = 0; tiled_cap_ = 0;
                GpuCheckStatus(kfx_alloc_pitched(&tiled_, &pitch, need, 1));
                tiled_cap_ = need;
            }
            GpuCheckStatus(kfx_slab_raycast_exact_tiled_color(depth.abi(), norm.abi(), img.abi(), tiled_, local.abi(), color->abi(), &layout, T_wc.m, &K.fu, near,
                                                              far, trunc_dist, subpix ? 1 : 0, tiles, comm, 0, 0, &last_rounds));
        } else if (raycast == Exact && tiles > 0) {
            const size_t need = kfx_slab_exact_tiled_scratch_bytes(depth.w, depth.h, tiles, comm->world);
            if (need > tiled_cap_) {
                size_t pitch;
                kfx_free(tiled_);
                tiled_ = 0; tiled_cap_ = 0;
                GpuCheckStatus(kfx_alloc_pitched(&tiled_, &pitch, need, 1));
                tiled_cap_ = need;
            }
            GpuCheckStatus(kfx_slab_raycast_exact_tiled(depth.abi(), norm.abi(), img.abi(), tiled_, local.abi(), &layout, T_wc.m, &K.fu, near, far, trunc_dist,
                                                        subpix ? 1 : 0, tiles, comm, 0, 0, &last_rounds));
        } else if (raycast == Exact) {
            GpuCheckStatus(kfx_slab_raycast_exact(depth.abi(), norm.abi(), img.abi(), (float*)state_, scratch_, local.abi(), &layout, T_wc.m,
                                                  &K.fu, near, far, trunc_dist, subpix ? 1 : 0, comm, 0, &last_rounds));
        } else if (raycast == ExactAllReduce) {
            GpuCheckStatus(kfx_slab_raycast_exact_allreduce(depth.abi(), norm.abi(), img.abi(), (float*)state_, scratch_, local.abi(), &layout, T_wc.m,
                                                            &K.fu, near, far, trunc_dist, subpix ? 1 : 0, comm, 0, &last_rounds));
        } else {
            if (color) RaycastSdf(depth, norm, img, local, *color, T_wc, K, near, far, trunc_dist, subpix);
            else RaycastSdf(depth, norm, img, local, T_wc, K, near, far, trunc_dist, subpix);
            if (merge == MergeDirect && comm->all_to_all && comm->all_gather) {
                const size_t need = kfx_slab_composite_direct_scratch_bytes(depth.w, depth.h, comm->world);
                if (need > strips_cap_) {
                    size_t pitch;
                    kfx_free(strips_);
                    strips_ = 0; strips_cap_ = 0;
                    GpuCheckStatus(kfx_alloc_pitched(&strips_, &pitch, need, 1));
                    strips_cap_ = need;
                }
                GpuCheckStatus(kfx_slab_composite_direct(depth.abi(), norm.abi(), img.abi(), strips_, comm, 0));
            } else {
                GpuCheckStatus(kfx_slab_composite(depth.abi(), norm.abi(), img.abi(), (long long*)key_, (float*)payload_, comm, 0));
            }
        }
    }

    // SaveMesh of this rank's part: the cubes whose lower plane it owns, every triangle bit-identical to the single-volume mesh's,
    // in emission order (include/kfx_mesh.h; the ghost planes must be current: Fuse leaves them so).  Writes filename + ".ply", with
    // the single-volume mesh's colours where the slab has a colour volume (as SaveMesh(filename, vol, volColor): when the whole colour
    // volume IsValid()); returns the triangle count.
    size_t SaveMesh(std::string filename) { return SaveRankMesh(filename, false, nullptr); }

    // SaveMesh's part of the mesh welded by lattice edge (include/kfx_mesh_index.h): the weld of this rank's triangles, so a vertex on a
    // slab boundary exists once per rank that uses it.  nvert, if given, receives the vertex count; returns the triangle count.
    size_t SaveMeshIndexed(std::string filename, size_t* nvert = nullptr) { return SaveRankMesh(filename, true, nvert); }

    // ... without its small components (MarchingCubes.h: SaveMeshIndexed(filename, vol, min_faces, largest)): refused.  A rank's mesh is
    // welded within the rank, so its components are cut at the slab boundaries: a surface that crosses one would count as two parts, each
    // smaller than the whole.  Filter the whole volume's mesh instead.
    size_t SaveMeshIndexed(std::string filename, size_t min_faces, bool largest, size_t* nvert = nullptr)
    {
        if (!min_faces && !largest) return SaveMeshIndexed(filename, nvert);
        throw std::invalid_argument("SlabVolume::SaveMeshIndexed: min_faces / largest are refused: a rank's mesh is welded within its rank, so its "
                                    "components are cut at the slab boundaries; filter the whole volume's mesh (roo::SaveMeshIndexed)");
    }

private:
    size_t SaveRankMesh(const std::string& filename, bool indexed, size_t* nvert)
    {
        const kfx_slab s = {layout.full_d, layout.s0, layout.full_zmin, layout.full_zmax};
        const bool with_color = color && local.w >= 8 && local.h >= 8 && layout.full_d >= 8;
        const mesh_detail::HostMesh m = mesh_detail::Extract(local.abi(), KFX_CELL_F32, &s, (int)layout.z0, (int)layout.z1, with_color ? color->abi() : nullptr, indexed);
        if (nvert) *nvert = m.nvert;
        return mesh_detail::WritePly(filename + ".ply", m);
    }

    static kfx_slab_layout MakeLayout(size_t d, const BoundingBox& bbox, kfx_comm* c, int ghost)
    {
        kfx_slab_layout L;
        GpuCheckStatus(kfx_slab_layout_init(&L, d, bbox.Min().z, bbox.Max().z, c->rank, c->world, ghost));
        return L;
    }
    void* key_; void* payload_; void* state_; void* scratch_; void* strips_; void* tiled_;
    size_t cap_, strips_cap_, tiled_cap_;
    void Reserve(size_t n)
    {
        if (n <= cap_) return;
        kfx_free(key_); kfx_free(payload_); kfx_free(state_); kfx_free(scratch_);
        size_t pitch;
        GpuCheckStatus(kfx_alloc_pitched(&key_, &pitch, n * sizeof(long long), 1));
        GpuCheckStatus(kfx_alloc_pitched(&payload_, &pitch, 5 * n * sizeof(float), 1));
        GpuCheckStatus(kfx_alloc_pitched(&state_, &pitch, KFX_RAY_STATE_PLANES * n * sizeof(float), 1));
        GpuCheckStatus(kfx_alloc_pitched(&scratch_, &pitch, kfx_slab_exact_scratch_bytes(n, 1), 1));
        cap_ = n;
    }
};

}
