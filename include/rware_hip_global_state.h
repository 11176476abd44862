/* rware_hip_global_state.h — part of the C-ABI of include/rware_hip.h, which includes this file: the critic's global state kept as one
 * byte record per env, and minibatches of global images gathered from such records and expanded on the device.  Do not include it on
 * its own: it needs rw_engine, and sits inside rware_hip.h's extern "C". */
#ifndef RWARE_HIP_GLOBAL_STATE_H
#define RWARE_HIP_GLOBAL_STATE_H
#ifndef RWARE_HIP_H
#error "include rware_hip.h, which includes this header"
#endif

/* -- the record: a published format ------------------------------------------------------------------------------------------ */
/* One record per env, uint8 [RB], RB = (H*W + 1 + 15) & ~15 (H = grid_h, W = grid_w; rw_global_record_bytes):
 *   byte c = y*W + x, c < H*W: the code of cell (x, y) — every layer of rw_global_image at once —
 *       bit 0     a shelf stands on the cell (SHELVES)
 *       bit 1     ... and it is a requested one (REQUESTS; a carried requested shelf lies under its carrier)
 *       bit 2     an agent stands on the cell (AGENTS; ACCESSIBLE is its inverse)
 *       bit 3     the cell is a goal (GOALS) — included, so a record is self-contained
 *       bit 4     AGENT_LOAD, bits 5..7 AGENT_DIRECTION (direction + 1, 0 for none): both on the MIRRORED cell, as the reference writes
 *                 them — `layer[ag.x, ag.y]` on an (H, W) array (rware/warehouse.py:1003, :1008), so an agent at (x, y) sets them in
 *                 byte x*W + y; the highest agent index wins a shared cell; an agent with x >= H or y >= W writes nothing there
 *   byte H*W: flags (enum rw_global_record_flags) —
 *       bit 0     some agent of this env has no mirrored cell (the reference raises IndexError for AGENT_DIRECTION)
 *       bit 1     some CARRYING agent has none (the reference raises for AGENT_LOAD)
 *   bytes H*W + 1 .. RB-1: zero.
 * A record costs about one byte per cell and step whichever layers, padding or element type the critic later asks for; a [T][B][RB]
 * tape of them is a rollout's global state. */
enum rw_global_record_flags { RW_GLOBAL_RECORD_NO_MIRROR = 1, RW_GLOBAL_RECORD_LOADED_NO_MIRROR = 2 };

/* RB for this engine's grid; a negative rw_status (RW_ERR_INVALID_ARG) for a NULL engine. */
int32_t rw_global_record_bytes(const rw_engine *eng);

/* records_dev[e][:] <- the record of env e, for all num_envs envs, from the engine's current state: the state RW_BUF_OBS describes at
 * that point of the stream (as rw_global_image).  records_dev: DEVICE uint8 [num_envs][RB], 16-byte aligned (RB is a multiple of 16: every
 * slot of a [T][B][RB] tape keeps the alignment); every byte of the num_envs * RB is written and nothing else.  Both flags are always
 * computed; the engine's status word is not touched (whether anybody asks for the two transposed layers is decided at gather time).
 * Any engine: every observation type and flag, 1 .. 127 agents, both shelf-cell widths.
 * Asynchrony: exactly one kernel launch on the engine's stream — no host synchronisation, no allocation, no copy; legal while the stream
 *   is being captured and replayed with the graph.
 * Errors: RW_ERR_INVALID_ARG for a NULL engine or records_dev, or a records_dev that is not 16-byte aligned. */
int rw_global_records(rw_engine *eng, void *records_dev);

/* out[i] <- the image rw_global_image would have written for the state record index[i] was taken from, for i < n_index.
 * records_dev: DEVICE uint8 [n_records][RB], 16-byte aligned — a [T][B][RB] tape as T*B records.  Only grid_h, grid_w and RB come from
 *   the engine: the records need not be this engine's current state, but must come from an engine of the same grid.
 * index_dev: DEVICE int32 [n_index], or int64 with RW_GLOBAL_INDEX64, aligned to its element; repeats are allowed.  NULL: the identity,
 *   n_index must equal n_records.  Only the kernel reads it, never the host.
 * layers, n_layers, pad_to_shape: as for rw_global_image — the layer list (duplicates allowed), the padding split and every value.
 * elem: enum rw_global_elem; RW_GLOBAL_F32 and RW_GLOBAL_U8 are rw_global_image's 0 and 1.  Every value is an integer in 0 .. 4 and exact
 *   in all four types.
 * out_dev: DEVICE [n_index][C'][H'][W'] of that element type, aligned to the element only: 16-byte stores on the 16-byte boundaries of
 *   the address, single elements in front of and behind them; every element is written and nothing else.
 * An index outside 0 .. n_records-1: that image is all zeros (ACCESSIBLE included), no record is read for it, and the next rw_sync
 *   returns RW_ERR_INVALID_ARG (the status bit of rw_snapshot_restore_indexed and rw_unpack_obs_gather: checked after
 *   RW_ERR_INVALID_ACTION and RW_ERR_INDEX, cleared with them).
 * AGENT_DIRECTION (AGENT_LOAD) among the layers and a GATHERED record with flag bit 0 (bit 1): the next rw_sync returns RW_ERR_INDEX; the
 *   image is what rw_global_image leaves in that case (that agent wrote nothing).  Records that are not gathered raise nothing.
 * Asynchrony: exactly one kernel launch on the engine's stream — no host synchronisation, no allocation, no host-to-device copy; legal
 *   while the stream is being captured (a replay reads the index and the records as they are at replay time).
 * Errors: RW_ERR_INVALID_ARG for a NULL engine, records_dev, layers or out_dev; a negative n_records or n_index; a NULL index_dev with
 *   n_index != n_records; an unknown elem or unknown flag bits; n_layers outside 1 .. 8, a layer outside 0 .. 6, a pad dimension smaller
 *   than the image; a pointer that is not aligned as said above; an image of more than 2^30 elements, more than 2^31 - 1 images or
 *   2^52 bytes of records (more than one launch holds: gather in slices).  n_index == 0 is RW_OK and writes nothing. */
enum rw_global_elem { RW_GLOBAL_F32 = 0, RW_GLOBAL_U8 = 1, RW_GLOBAL_F16 = 2, RW_GLOBAL_BF16 = 3 };
enum rw_global_flags { RW_GLOBAL_INDEX64 = 1 };   /* index_dev holds int64, else int32 */
int rw_global_image_gather(rw_engine *eng, const uint8_t *records_dev, int64_t n_records, const void *index_dev, int64_t n_index,
                           const int32_t *layers, int32_t n_layers, const int32_t *pad_to_shape, int32_t elem, int32_t flags, void *out_dev);

#endif /* RWARE_HIP_GLOBAL_STATE_H */
