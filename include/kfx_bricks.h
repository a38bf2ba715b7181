/* kfx_bricks.h -- sparse brick snapshots: the 8 x 8 x 8 bricks of a BoundedVolume that hold anything, packed on the device, and
 * put back byte for byte.  What a moving volume spills when it shifts (kfx_shift.h), what a checkpoint of a mostly never-observed
 * volume costs, what a slab gather moves.  Same library (libkfx.so); kept out of kfx.h.
 *
 * The brick grid of a volume or of any view of one (SubVolume, Z-slab view; no alignment of the origin is asked for) starts at the
 * view's cell (0, 0, 0): nbx = ceil(w / 8) bricks along x, nby = ceil(h / 8), nbz = ceil(d / 8), brick id = (bz * nby + by) * nbx + bx.
 * Where a dimension is no multiple of 8 the last bricks are partial.  A view may hold 2^31 - 1 bricks at the most.
 *
 * LIVE.  A brick is live if any of its cells inside the view differs BITWISE from the fill cell: for KFX_CELL_F32 / KFX_CELL_F16 the
 * bytes kfx_sdf_reset(vol, fill) / kfx_sdf_reset_h(vol, fill) write, for KFX_CELL_COLOR fill itself -- the bytes kfx_volume_shift
 * fills with, from the same function.  Words are compared, never floats: a NaN of another payload is a difference, so is -0.0
 * against 0.0, so is a cell whose val equals the fill's while its w does not.
 *
 *   kfx_bricks_plan    classifies every brick in one streaming read of the view, scans the flags in ascending id and blocks until
 *                      *n_live is in host memory (one 8-byte read-back).
 *   kfx_bricks_pack    writes ids[n_live], uint32, ascending, and cells[n_live][8][8][8], x fastest, in the cell's bytes, verbatim;
 *                      positions of a partial brick outside the view hold the fill bytes.  Takes the plan's scratch unchanged and
 *                      the plan's n_live: it reads the planned number back from the scratch (8 bytes) and refuses another with
 *                      KFX_E_RANGE.  The volume must not change between the two calls.  Nothing is written beyond n_live entries.
 *   kfx_bricks_unpack  writes the cells inside the view of the n listed bricks from the payload and nothing else: no other brick,
 *                      no pitch padding, no neighbour of a sub-view.  ids must ascend strictly; an id >= the view's brick count
 *                      is skipped by the kernel; with a repeated id, which copy wins is unspecified.  n == 0 launches nothing.
 *
 *   ids, cells  device memory of the caller; ids 4-byte aligned, cells 16-byte aligned (one brick: 512 cells = 4096 bytes of
 *               KFX_CELL_F32, 2048 bytes of the 4-byte cells).
 *   scratch     device memory of the caller, 256-byte aligned, of kfx_bricks_scratch_bytes() bytes; the library never allocates.
 *               With nb = nbx * nby * nbz bricks and nblk = ceil(nb / 256) scan blocks:
 *                   256 + round256(nb) + 2 * round256(4 * nblk)      (round256: up to a multiple of 256)
 *               -- a header, one flag byte per brick, the scan blocks' counts and their offsets; nothing per cell.  512^3 cells:
 *               270 592 bytes.
 *
 * Returns 0 or KFX_E_*: a null volume, scratch, n_live or -- with entries to move -- ids / cells KFX_E_NULL; an unknown cell kind
 * KFX_E_RANGE; the volume's own rules (KFX_E_SHAPE / KFX_E_ALIGN; every dimension >= 1, as for the shift); more than 2^31 - 1 bricks
 * or entries KFX_E_RANGE; a scratch below kfx_bricks_scratch_bytes() KFX_E_SHAPE; a misaligned scratch, ids or cells KFX_E_ALIGN --
 * all before any HIP call; then, from kfx_bricks_pack, an n_live that is not the plan's KFX_E_RANGE, before any launch. */
#ifndef KFX_BRICKS_H
#define KFX_BRICKS_H

#include "kfx_shift.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch a plan of these arguments needs; 0 if the arguments are refused */
size_t kfx_bricks_scratch_bytes(const kfx_volume* vol, int cell);
int kfx_bricks_plan(const kfx_volume* vol, int cell, float fill, void* scratch, size_t scratch_bytes, unsigned long long* n_live, kfx_stream stream);
int kfx_bricks_pack(const kfx_volume* vol, int cell, float fill, const void* scratch, size_t scratch_bytes, unsigned long long n_live, unsigned* ids,
                    void* cells, kfx_stream stream);
int kfx_bricks_unpack(const kfx_volume* vol, int cell, const unsigned* ids, const void* cells, unsigned long long n, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_BRICKS_H */
