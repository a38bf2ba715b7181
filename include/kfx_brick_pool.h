/* kfx_brick_pool.h -- a brick pool: device memory of the caller that keeps the 8 x 8 x 8 bricks a moving volume leaves behind
 * (kfx_shift.h, kfx_bricks.h) under world brick keys, and gives them back -- spill and restore are stream-ordered launches that never
 * touch the host.  Same library (libkfx.so); kept out of kfx.h.
 *
 * LAYOUT.  A pool holds `capacity` bricks of one cell kind (KFX_CELL_F32, KFX_CELL_F16, KFX_CELL_COLOR; cb = 8, 4, 4 bytes per cell).
 * Its layout depends on (cell, capacity) alone; every part starts on a multiple of 256 bytes:
 *     header   256 bytes: free_n, spilled, restored, dropped as uint64 at bytes 0, 8, 16, 24 (the last three cumulative), then the
 *              record {cell, capacity} as uint32 at bytes 32 and 36
 *     keys     capacity x 16 bytes {bx, by, bz, state} as int32: state 1 = occupied, 0 = free      at byte 256
 *     free     capacity x uint32: the stack of free slot numbers, free[0 .. free_n)                at 256 + round256(16 capacity)
 *     cells    capacity x 512 cells, x fastest, the cell's bytes verbatim                          after round256(4 capacity) more
 *     kfx_brick_pool_bytes = 256 + round256(16 capacity) + round256(4 capacity) + 512 cb capacity      (round256: up to a multiple of 256)
 * Every call takes (pool, pool_bytes, cell, capacity) and derives the layout from these arguments; the record in the header is never
 * read back to validate a call.  The library never allocates.  The bytes of a pool are a function of the sequence of calls: slots are
 * handed out by a scan in ascending order, never by an atomic.
 *
 * KEYS.  Brick (i, j, k) of a view's own brick grid (kfx_bricks.h: ceil(dim / 8) bricks per axis from the view's cell (0, 0, 0),
 * partial last bricks allowed) has the world key key0 + (i, j, k); the key range of the view is key0 .. key0 + (nbx, nby, nbz) - 1.
 *
 *   kfx_brick_pool_init      every slot free, free[i] = capacity - 1 - i (slot 0 is handed out first), the counters zero.
 *   kfx_brick_pool_spill     first discards every brick the pool holds whose key lies in the view's key range (a key is in the pool at
 *                            most once; a later spill of a key replaces the earlier one).  Then the live bricks of the view (LIVE as
 *                            kfx_bricks.h: bitwise against the fill cell) go in, in ascending brick id: the r-th live brick takes the
 *                            slot free[free_n - 1 - r]; cells of a partial brick outside the view hold the fill bytes.  A brick with
 *                            r >= free_n is DROPPED: nothing is written for it and `dropped` counts it.  The view is not modified.
 *   kfx_brick_pool_restore   takes the occupied slots whose key lies in the view's key range, in ascending slot number: the cells of
 *                            that brick inside the view are written from the payload and nothing else is (as kfx_bricks_unpack); the
 *                            slot becomes free and the i-th such slot is pushed to free[free_n + i].
 *   kfx_brick_pool_discard   the discard step on its own, for a box of nb[0] x nb[1] x nb[2] keys from key0: restore without the copy
 *                            (and without counting into `restored`).
 *   kfx_brick_pool_stats     the one blocking call: reads 32 bytes back; out = {occupied, spilled, restored, dropped}.
 *   kfx_brick_pool_gather    cells_out[i][512 cells] = the payload of slot slots[i], device to device; a slot >= capacity is skipped.
 *                            With a plain copy of the keys block this gives a caller the contiguous lists kfx_mesh_bricks.h and
 *                            kfx_raycast_bricks.h take; the payload never crosses to the host.
 * None of spill, restore, discard and gather reads anything back: their grids cover every brick of the view (every slot of the
 * pool) and the kernels read the counts from the scratch and the header.
 *
 *   scratch   device memory of the caller, 256-byte aligned; one scratch of kfx_brick_pool_scratch_bytes(view, cell, capacity) bytes
 *             serves spill, restore and (any box) discard.  With n = max(bricks of the view, capacity), nblk = ceil(n / 256):
 *                 256 + round256(n) + 2 * round256(4 * nblk) + round256(4 * n)
 *             -- a header, a flag byte per entry, the scan blocks' counts and offsets, a uint32 list.  A discard needs n = capacity.
 *             Its contents mean nothing between calls.
 *   slots     device memory, 4-byte aligned; cells_out device memory, 16-byte aligned (n == 0: nothing is asked of them).
 *
 * Returns 0 or KFX_E_*, every refusal before any HIP call, in this order: a null pool, view (or view->ptr), key0, nb, out or scratch
 * KFX_E_NULL; an unknown cell kind KFX_E_RANGE; capacity 0 or above 2^31 - 1 KFX_E_RANGE; a pool below kfx_brick_pool_bytes()
 * KFX_E_SHAPE; a pool not aligned to 256 bytes KFX_E_ALIGN; the view: the volume's own rules (KFX_E_SHAPE / KFX_E_ALIGN, every
 * dimension >= 1; more than 2^31 - 1 bricks KFX_E_RANGE; a discard: an nb below 1 or more than 2^31 - 1 keys KFX_E_SHAPE / KFX_E_RANGE); a
 * scratch below kfx_brick_pool_scratch_bytes() KFX_E_SHAPE; a scratch not aligned to 256 bytes KFX_E_ALIGN; a key range that leaves
 * int32 KFX_E_RANGE; gather: more than 2^31 - 1 entries KFX_E_RANGE, null lists KFX_E_NULL, misaligned lists KFX_E_ALIGN.
 *
 * MEMORY SAFETY.  A slot number read from free[] or from a list is used only if it is below capacity, free_n only up to capacity, a
 * brick coordinate derived from a key only if it lies inside the view's grid: a pool whose bytes were overwritten gives unspecified
 * contents, never an access outside the pool, the scratch or the view. */
#ifndef KFX_BRICK_POOL_H
#define KFX_BRICK_POOL_H

#include "kfx_bricks.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of a pool / of the scratch; 0 if the arguments are refused */
size_t kfx_brick_pool_bytes(int cell, unsigned long long capacity);
size_t kfx_brick_pool_scratch_bytes(const kfx_volume* view, int cell, unsigned long long capacity);
int kfx_brick_pool_init(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, kfx_stream stream);
int kfx_brick_pool_spill(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const kfx_volume* view, float fill, const int key0[3],
                         void* scratch, size_t scratch_bytes, kfx_stream stream);
int kfx_brick_pool_restore(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const kfx_volume* view, const int key0[3], void* scratch,
                           size_t scratch_bytes, kfx_stream stream);
int kfx_brick_pool_discard(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const int nb[3], const int key0[3], void* scratch,
                           size_t scratch_bytes, kfx_stream stream);
int kfx_brick_pool_stats(const void* pool, size_t pool_bytes, int cell, unsigned long long capacity, unsigned long long out[4], kfx_stream stream);
int kfx_brick_pool_gather(const void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const unsigned* slots, unsigned long long n,
                          void* cells_out, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_BRICK_POOL_H */
