/* rware_hip_restore.h — part of the C-ABI of include/rware_hip.h, which includes this file: restoring or cloning single envs from a snapshot
 * by a device index array.  Do not include it on its own: it needs rw_engine and rw_snapshot, and sits inside rware_hip.h's extern "C". */
#ifndef RWARE_HIP_RESTORE_H
#define RWARE_HIP_RESTORE_H
#ifndef RWARE_HIP_H
#error "include rware_hip.h, which includes this header"
#endif

/* -- restore or clone single envs from a snapshot, by index, on the device ----------------------- */
/* env e <- the state the snapshot holds for env src_index_dev[e]; -1: env e keeps its current state.
 * src_index_dev: DEVICE int32 [num_envs], 4-byte aligned; 0 .. num_envs-1 names a snapshot slot, repeats are allowed (many envs may take
 *   one slot: broadcast a start state, branch children off one env).  Only the kernel reads it, never the host.
 * Copied, per restored env: exactly what a snapshot holds for one env — the packed agent records, the counter record (steps, inactive,
 *   the pending NEXT_STEP reset), RW_BUF_QUEUE, the six fields of RW_BUF_RNG, RW_BUF_AGENT_MSG, RW_BUF_STAT_* and RW_BUF_EP_* where
 *   their flags exist, the shelf layer.  RW_BUF_REWARDS, RW_BUF_TERMINATED and RW_BUF_TRUNCATED are outputs of a step: they are left
 *   as they are, as rw_snapshot_restore leaves them.
 * flags: RW_RESTORE_KEEP_RNG — the six RNG fields of EVERY env stay as they are, bit for bit, so clones of one state draw different
 *   request replacements.  Without it clones are identical and stay identical under identical actions (rw_seed_device afterwards
 *   separates them).  Any other bit: RW_ERR_INVALID_ARG.
 * Results: behind the copy the call makes the observation launch rw_snapshot_restore makes, so RW_BUF_OBS / RW_BUF_OBS_PACKED / the uint8
 *   rows, RW_BUF_FEATURES and RW_BUF_ACTION_MASK of all envs are current, in the engine's own format; the derived views are rebuilt
 *   when next asked for.
 * Asynchrony: one gather launch and the observation launch on the engine's stream — no host synchronisation, no allocation, no
 *   host-to-device copy; legal while the stream is being captured and replayed with the graph (a replay reads the index array's
 *   contents at replay time).  The snapshot and the index array must stay valid until the work has run.
 * An index outside -1 .. num_envs-1: that env is left untouched, nothing out of bounds is read, and the next rw_sync returns
 *   RW_ERR_INVALID_ARG (checked after RW_ERR_INVALID_ACTION and RW_ERR_INDEX, cleared with them).
 * Errors: RW_ERR_INVALID_ARG for a NULL engine, snapshot or index array, an index pointer that is not 4-byte aligned, unknown flag bits. */
enum rw_restore_flags { RW_RESTORE_KEEP_RNG = 1 };
int rw_snapshot_restore_indexed(rw_engine *eng, const rw_snapshot *snap, const int32_t *src_index_dev, int32_t flags);

#endif /* RWARE_HIP_RESTORE_H */
