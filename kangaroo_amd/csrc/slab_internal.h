// slab_internal.h -- what slab.hip offers slab_frame.hip beyond include/kfx_slab.h: the layout check they share, and the exact hand-over in
// its two halves, so that a frame object can leave the final exchange of frame k on its own stream and communicator under frame k + 1's march.
#pragma once
#include "host_args.h"
#include "../../include/kfx_slab.h"
#include "../../include/kfx_slab_color.h"

namespace kfx {
// a rank's local volume and communicator are the ones the layout was made for (all three non-null); `what` names the entry point
inline int check_layout(const kfx_volume* local, const kfx_slab_layout* L, const kfx_comm* comm, const char* what)
{
    if (local->d != L->s1 - L->s0 || comm->rank != L->rank || comm->world != L->world)
        return fail_rule(what, KFX_E_SHAPE, "volume / communicator do not match the layout");
    return 0;
}

// the buffers of one final exchange: this rank's contributions, the received / gathered strips, this rank's merged strip, the count of
// pixels left without a final status; S: pixels per image strip of the exchange (0 for one rank)
struct ExactFinalBufs { int* contrib; int* gathered; int* mine; int* open; size_t S; };
size_t exact_final_carve(ExactFinalBufs& b, void* mem, size_t w, size_t h, int world);   // returns ints; mem may be null: sizes only
// the parts of kfx_slab_raycast_exact_tiled's scratch buffer
struct TiledScratch {
    size_t P, n;       // plane stride of a tile (pixels), pixels of the image
    int R, T;          // rows per tile, tiles
    int *M, *Rz, *from_lo, *from_hi, *fin;
    ExactFinalBufs own;   // the final exchange's buffers inside the scratch
};
size_t tiled_layout(TiledScratch& t, void* scratch, size_t w, size_t h, int tiles, int world);   // returns ints; scratch may be null
// kfx_slab_raycast_exact_tiled[_color] = exact_tiled: the argument checks, exact_tiled_march + exact_tiled_finalise on one stream with the
// scratch's own buffers, and -- without h_open -- the read-back of the open count.  color_local: this rank's colour slab or null.
int exact_tiled(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, void* scratch, const kfx_volume* local, const kfx_volume* color_local,
                const kfx_slab_layout* L, const float T_wc[12], const float K[4], float near, float far, float trunc_dist, int subpix, int tiles, kfx_comm* comm,
                kfx_stream stream, int* h_open, int* steps_out);
// the march leaves this rank's contributions in `into`; the finalise exchanges `from` and writes the images (w x h = img's size)
int exact_tiled_march(const TiledScratch& t, const ExactFinalBufs& into, const kfx_volume* local, const kfx_slab_layout* L, const float T_wc[12],
                      const float K[4], float near, float far, float trunc_dist, int subpix, int w, int h, kfx_comm* comm, kfx_stream stream, int* steps_out,
                      const kfx_volume* color_local = nullptr);
int exact_tiled_finalise(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const ExactFinalBufs& from, kfx_comm* comm, kfx_stream stream,
                         int* h_open);
}
