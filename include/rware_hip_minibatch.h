/* rware_hip_minibatch.h — part of the C-ABI of include/rware_hip.h, which includes this file: gathering packed observation rows by a
 * device index array and unpacking them, in one launch, into float32, float16 or bfloat16.  Do not include it on its own: it needs
 * rw_engine, and sits inside rware_hip.h's extern "C". */
#ifndef RWARE_HIP_MINIBATCH_H
#define RWARE_HIP_MINIBATCH_H
#ifndef RWARE_HIP_H
#error "include rware_hip.h, which includes this header"
#endif

/* -- gather and unpack packed observation minibatches on the device ------------------------------ */
/* out[i][r][:] <- the unpacked row packed[index[i]][r][:], for i < n_index, r < rows_per_group: what a learner does with a packed rollout
 * when it draws a minibatch, without the gathered copy and the intermediates of doing it in tensor ops.
 * packed_dev: DEVICE uint32 [n_groups][rows_per_group][PW], 4-byte aligned — a [T][B][N][PW] tape as T*B groups of N rows, RW_BUF_OBS_PACKED
 *   as num_envs groups of N rows, or any rows with rows_per_group 1.  PW is 1 + ceil(L / 32) words with L = rw_info.obs_length, as
 *   for rw_unpack_obs; the shape facts (L, grid size, normalised_coordinates) are the engine's, which need not have RW_OBS_PACKED itself.
 * index_dev: DEVICE int32 [n_index], or int64 with RW_UNPACK_INDEX64, aligned to its element; output group i is source group index[i],
 *   repeats are allowed.  NULL: the identity, n_index must equal n_groups — a whole-array unpack into the chosen element type.  Only the
 *   kernel reads it, never the host.
 * out_dev: DEVICE [n_index][rows_per_group][L] elements of `elem`, aligned to the element; an output that starts on a 16-byte boundary is
 *   written with 16-byte stores, any other with element stores.
 * Values: RW_UNPACK_F32 is bit for bit what rw_unpack_obs and RW_BUF_OBS give.  RW_UNPACK_F16 / RW_UNPACK_BF16 are that float32 value
 *   rounded to nearest even: 0 and 1 are exact, only the two coordinates round (float16 holds integers up to 2048 exactly, bfloat16 up
 *   to 256; a normalised coordinate v / (dim - 1) is inexact in both).
 * An index outside 0 .. n_groups-1: that output group is all zeros, nothing out of bounds is read, and the next rw_sync returns
 *   RW_ERR_INVALID_ARG (the status bit of rw_snapshot_restore_indexed: checked after RW_ERR_INVALID_ACTION and RW_ERR_INDEX, cleared
 *   with them).
 * Asynchrony: exactly one kernel launch on the engine's stream — no host synchronisation, no allocation, no host-to-device copy; legal
 *   while the stream is being captured and replayed with the graph (a replay reads the index array's contents at replay time).  All
 *   three arrays must stay valid until the work has run.
 * Errors: RW_ERR_UNSUPPORTED for an IMAGE / IMAGE_DICT engine (as rw_unpack_obs).  RW_ERR_INVALID_ARG for a NULL engine, packed_dev or
 *   out_dev; a negative n_groups or n_index, rows_per_group < 1; an unknown elem or unknown flag bits; a NULL index_dev with
 *   n_index != n_groups; a pointer that is not aligned as said above; more output than one launch holds (2^31 - 1 workgroups of 4 KiB:
 *   unpack in slices).  n_index == 0 is RW_OK and writes nothing. */
enum rw_unpack_elem { RW_UNPACK_F32 = 0, RW_UNPACK_F16 = 1, RW_UNPACK_BF16 = 2 };
enum rw_unpack_flags { RW_UNPACK_INDEX64 = 1 };   /* index_dev holds int64, else int32 */
int rw_unpack_obs_gather(rw_engine *eng, const uint32_t *packed_dev, int64_t n_groups, int32_t rows_per_group,
                         const void *index_dev, int64_t n_index, int32_t elem, int32_t flags, void *out_dev);

#endif /* RWARE_HIP_MINIBATCH_H */
