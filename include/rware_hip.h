/*
 * rware_hip.h — C-ABI of the MI355X-native vectorised RWARE step engine.
 *
 * This is the drop-in boundary for ONE path of semitable/robotic-warehouse: the per-step hot
 * path of `rware.warehouse.Warehouse` (reset / step / FLATTENED observation), batched over
 * `num_envs` independent warehouses resident in HBM on one HIP device.  The reference has no
 * native code, so there is no existing FFI to mirror; each entry point below cites the Python
 * interface it replaces.  The Python binding a maintainer would add is in INTEGRATION.md; the
 * in-tree one is robotic-warehouse_amd/_capi.py.
 *
 * Conventions
 *   - plain C types only; every call returns an `int` status (RW_OK == 0, negatives are errors)
 *     and never throws or aborts across the boundary; `rw_last_error` gives the message.
 *   - the engine owns all device memory for its lifetime; pointers from `rw_get_buffer` are
 *     borrowed, stable until `rw_destroy`, and the obs/reward/terminated buffers are overwritten
 *     by the next step.  Callers own the action arrays they pass in.
 *   - one engine == one HIP device + one stream.  Calls on one engine are not re-entrant;
 *     different engines (one per GPU) may be driven from different host threads.
 *   - all work is enqueued asynchronously on the engine's stream; `rw_sync` waits for it.
 *   - env index e, agent index i (agent id = i+1), cell index c = y*W + x.
 */
#ifndef RWARE_HIP_H
#define RWARE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (since 3): RW_OBS_PACKED in rw_stream_flags, RW_BUF_OBS_PACKED (RW_BUF_KIND_COUNT 22 -> 23), rw_info.obs_packed appended (the struct
 * grows by 8 bytes), rw_unpack_obs, a 16th element (`packed`) in rw_jit_probe's shape.  Everything else is unchanged.
 * Still 4, a compatible addition: RW_EPISODES_ON in rw_stream_flags, RW_BUF_EP_RETURN .. RW_BUF_EP_COUNT appended (RW_BUF_KIND_COUNT 23 -> 28;
 * all five empty without the flag), and rw_info.stats read as a bit set — bit 0 RW_STATS_ON, bit 1 RW_EPISODES_ON — so an engine with only
 * the old flag still reports 1; rw_info keeps its size.
 * Still 4, a compatible addition: RW_ACTION_MASK_ON in rw_stream_flags, RW_BUF_ACTION_MASK appended (RW_BUF_KIND_COUNT 28 -> 29; empty
 * without the flag), bit 2 of rw_info.stats; rw_info keeps its size, no new entry point.
 * Still 4, a compatible addition: RW_OBS_IMAGE_U8 in rw_stream_flags — the elements of RW_BUF_OBS of an IMAGE / IMAGE_DICT engine become
 * uint8 (same kind, same shape, a quarter of the bytes; RW_BUF_KIND_COUNT stays 29), rw_info.obs_packed reads 2 for such an engine;
 * rw_info keeps its size, no new entry point.
 * Still 4, a compatible addition: two entry points, rw_seed_device and rw_reset_device (seeding and masked reset from DEVICE arrays,
 * enqueue only); no struct, flag or buffer kind changes, rw_reset itself is unchanged.
 * Still 4, a compatible addition: one entry point, rw_global_image (Warehouse.get_global_image built on the device into an array of the
 * caller's, enqueue only); no struct, flag or buffer kind changes (RW_BUF_KIND_COUNT stays 29).
 * Still 4, a compatible addition: RW_TIME_LIMIT_TRUNCATES in rw_stream_flags (RW_BUF_TRUNCATED becomes live with it; no new buffer kind,
 * RW_BUF_KIND_COUNT stays 29), bit 3 of rw_info.stats, and two entry points, rw_step_many_device2 and rw_read_outputs2 (their namesakes
 * plus the truncated flags); rw_info keeps its size, rw_step_many_device and rw_read_outputs are unchanged.
 * Still 4, a compatible addition: rw_config.n_agents takes 1..127 (was 1..64).  65 .. 127 agents always run the generic kernel
 * (rw_info.build_kind 0, no run-time build, not even with RW_JIT_FORCE; rw_jit_log says so), by default on workgroups of 4 envs, and
 * envs_per_workgroup * n_agents must stay below 2355 there.  128 and more stay RW_ERR_INVALID_ARG: the kernels' per-cell agent layer
 * holds id | 0x80 (loaded) in one byte.  No struct, flag, buffer kind or entry point changes.
 * Still 4, a compatible addition: one entry point, rw_snapshot_restore_indexed (single envs restored or cloned from a snapshot by a
 * DEVICE index array, enqueue only) with its own flag word rw_restore_flags, both declared in rware_hip_restore.h; no struct, stream flag or buffer kind changes
 * (RW_BUF_KIND_COUNT stays 29), rw_snapshot_restore itself is unchanged.
 * Still 4, a compatible addition: one entry point, rw_unpack_obs_gather (packed rows gathered by a DEVICE index array and unpacked into
 * float32, float16 or bfloat16 in one launch, enqueue only) with its enums rw_unpack_elem and rw_unpack_flags, declared in
 * rware_hip_minibatch.h; no struct, stream flag or buffer kind changes, rw_unpack_obs itself is unchanged.
 * Still 4, a compatible addition: three entry points, rw_global_record_bytes, rw_global_records (the code byte per cell that
 * rw_global_image expands, written as one uint8 record per env, enqueue only) and rw_global_image_gather (records gathered by a DEVICE
 * index array and expanded into float32, uint8, float16 or bfloat16 images in one launch, enqueue only) with their enums rw_global_elem,
 * rw_global_flags and rw_global_record_flags, declared in rware_hip_global_state.h; no struct, stream flag or buffer kind changes,
 * rw_global_image itself is unchanged.
 * Still 4, a compatible addition: one entry point (advantages and returns, GAE(lambda), from a rollout's reward, flag and value tapes in
 * one launch, enqueue only) with its argument struct rw_gae_args and its enum rw_gae_flags, declared in rware_hip_advantages.h; no
 * other struct, stream flag or buffer kind changes. */
#define RW_ABI_VERSION 4

typedef struct rw_engine rw_engine;

enum rw_status {
    RW_OK = 0,
    RW_ERR_INVALID_ARG = -1,    /* bad config / null pointer / size mismatch                     */
    RW_ERR_INVALID_ACTION = -2, /* an action outside 0..4 was seen (reference: Action(a) raises
                                   ValueError, rware/warehouse.py:814); sticky until rw_sync      */
    RW_ERR_HIP = -3,            /* a HIP runtime call failed                                      */
    RW_ERR_UNSUPPORTED = -4,    /* feature outside the accelerated path (DICT observations, ...)  */
    RW_ERR_NO_DEVICE = -5,      /* no usable HIP device: there is NO CPU fallback                 */
    RW_ERR_INDEX = -6,          /* an AGENT_DIRECTION / AGENT_LOAD image layer met an agent at
                                   x >= grid_h or y >= grid_w, where the reference raises IndexError
                                   (rware/warehouse.py:552,558); sticky until rw_sync             */
    RW_ERR_SELFTEST = -7        /* rw_selftest: this device / toolchain breaks an assumption the kernels are built on */
};

/* rware/warehouse.py:31-36 */
enum rw_action { RW_NOOP = 0, RW_FORWARD = 1, RW_LEFT = 2, RW_RIGHT = 3, RW_TOGGLE_LOAD = 4 };
/* rware/warehouse.py:39-43 */
enum rw_direction { RW_UP = 0, RW_DOWN = 1, RW_DIR_LEFT = 2, RW_DIR_RIGHT = 3 };
/* rware/warehouse.py:46-49 */
enum rw_reward_type { RW_REWARD_GLOBAL = 0, RW_REWARD_INDIVIDUAL = 1, RW_REWARD_TWO_STAGE = 2 };

/* rware/warehouse.py:52-56.  DICT (nested Python objects) is FLATTENED at this boundary: the host layer
 * un-flattens the same vector (rware/warehouse.py:432-443). */
enum rw_observation_type { RW_OBS_FLATTENED = 1, RW_OBS_IMAGE = 2, RW_OBS_IMAGE_DICT = 3 };
/* rware/warehouse.py:59-70.  AGENT_DIRECTION and AGENT_LOAD are reproduced as the reference writes them:
 * with transposed indices (`layer[ag.x, ag.y]` on an (H, W) array, :552/:558), i.e. the value lands on the
 * mirrored cell, and a state in which the reference raises IndexError is reported as RW_ERR_INDEX by the
 * next rw_sync (every registered layout has H > W, so that happens as soon as an agent reaches y >= W). */
enum rw_image_layer { RW_LAYER_SHELVES = 0, RW_LAYER_REQUESTS = 1, RW_LAYER_AGENTS = 2, RW_LAYER_AGENT_DIRECTION = 3,
                      RW_LAYER_AGENT_LOAD = 4, RW_LAYER_GOALS = 5, RW_LAYER_ACCESSIBLE = 6 };

/* What a step does with an env whose episode ended (Gymnasium vector-env autoreset modes).
 * The reference env itself never resets (the caller calls reset()); DISABLED reproduces that. */
enum rw_autoreset {
    RW_AUTORESET_DISABLED = 0,
    RW_AUTORESET_NEXT_STEP = 1, /* the step after `terminated` performs reset(): action ignored,
                                   reward 0, terminated 0 (Gymnasium >= 1.0 default)              */
    RW_AUTORESET_SAME_STEP = 2  /* the terminating step returns the reset observation; the terminal
                                   observation is kept in RW_BUF_FINAL_OBS (Gymnasium's
                                   info["final_obs"])                                             */
};

/* How `rw_config.stream` is read.  A hipStream_t of NULL is also the handle of the device's default
 * ("null") stream — the stream frameworks such as PyTorch run on unless told otherwise — so "NULL == make
 * your own" cannot express "enqueue on the default stream".  RW_STREAM_USE_GIVEN takes the handle
 * literally: NULL then means the default stream, and the engine's launches are ordered with everything
 * else the caller enqueues there (a policy writing the action tensor before, a learner reading the
 * observation tensor after) without any explicit synchronisation. */
enum rw_stream_flags {
    RW_STREAM_USE_GIVEN = 1,
    /* How the observation stream is stored.  Default (neither bit): the engine decides — non-temporal stores (the observation
     * lines are written once and not re-read by the engine: with the hint they do not displace the state the next step
     * reads) wherever that was measured faster, which is everywhere except workgroups with a large observation chunk
     * (16 agents) below the Infinity Cache size.  A learner that reads the observations right behind the step finds
     * non-temporal lines in HBM rather than in the cache: RW_OBS_STORES_CACHED keeps them cached, RW_OBS_STORES_STREAM forces
     * the hint.  (A/B runs: RWARE_OBS_STORES=cached|stream in the environment, honoured with RWARE_HOOKS=1 — csrc/rware_hooks.h.) */
    RW_OBS_STORES_CACHED = 2,
    RW_OBS_STORES_STREAM = 4,
    /* Run-time specialisation.  A task without an ahead-of-time exact-shape kernel build — a `layout=` string, column_height
     * != 8, sensor_range 2..5, more than 19 agents (rware/warehouse.py:146-170; ids of rware/__init__.py:83-175) — gets one
     * compiled by rw_create through hipRTC (a few seconds; cached on disk under $RWARE_JIT_CACHE or ~/.cache/rware_amd/jit)
     * when the batch has at least 4096 envs; without hipRTC, or when the compile fails, the ahead-of-time generic kernel
     * runs (rw_info.jit, rw_jit_log say what happened).  RW_JIT_OFF: never.  RW_JIT_FORCE: always — small batches and shapes
     * that have an ahead-of-time build included (tests, A/B).  (A/B runs: RWARE_JIT=off|force with RWARE_HOOKS=1.) */
    RW_JIT_OFF = 8,
    RW_JIT_FORCE = 16,
    /* The chunk-pipelined persistent build of the per-step kernel (round 5): instead of one workgroup per chunk of envs, as many
     * workgroups as the GPU holds at once walk the chunks, the agent phases of the next chunk running beside the observation stores
     * of the current one and the chunk after that already on its way into LDS.  Measured SLOWER than the classic launch on every
     * configuration (profiles/EXPERIMENTS.md, round 5), so: rw_create NEVER picks it by itself, and the default library does not even
     * contain it — only a `make PIPE=1` build does (rware_static_table.h, group 18: the BASELINE shapes and two agent-count-static
     * ones).  RW_PIPE_ON: use it where such a build exists for the shape (FLATTENED, no messages, ahead-of-time kernels, batch a multiple of
     * its chunk size), else the classic kernel runs and rw_jit_log() says why; rw_info.pipe_workgroups != 0 tells which one runs.
     * RW_PIPE_OFF: never (the default).  (A/B runs: RWARE_PIPE=0|1 with RWARE_HOOKS=1.) */
    RW_PIPE_OFF = 32,
    RW_PIPE_ON = 64,
    /* Event counters (SURVEY.md §5 "metrics"): with RW_STATS_ON the engine keeps two running totals per env in RW_BUF_STAT_DELIVERIES and
     * RW_BUF_STAT_FAILED_MOVES (below) — off by default, and the reference's `info` stays {} either way (rware/warehouse.py:746-747).
     * Counted by the service wavefront beside the observation stores (re-derived from what the state write-back holds; nothing is added
     * to the agent phases), in every launch form: rw_step*, fused rollouts, tapes, HIP graphs, rw_multi.
     * Which kernels run with it: the ahead-of-time exact-shape builds do not carry the counting code, so below 4096 envs, with RW_JIT_OFF
     * or without hipRTC the generic kernel runs (rw_info.build_kind == 0); from 4096 envs on rw_create compiles an exact-shape build with
     * the counters through hipRTC at construction (seconds; cached on disk as described at RW_JIT_OFF; rw_info.jit says which happened). */
    RW_STATS_ON = 128,
    /* Wavefront priority (rw_info.wave_priority): the launches run the dependent chain in front of their first observation store at raised
     * priority by rw_create's measured rule (on, except the per-step launches of 13 .. 16 agents at sensor_range 1 on 8-env workgroups
     * beyond half a round of workgroups, and steps of 200 MB of observations and more).  RW_PRIO_OFF: never — what rware_amd.make_pipelines
     * asks for when a sub-batch has 8192 envs or fewer: with TWO launches in flight the raised chain of one takes the issue slots of the
     * other's store phase, which is what fills the gap (two pipelines of 8192 envs, per step of the whole batch: small-8ag 7.9 us without
     * against 9.1 with, small-10ag 10.7 / 11.9, medium-13ag 13.4 / 15.4; profiles/r06_pipelines_prio.txt).  RW_PRIO_ON: always (per-step
     * launches and fused rollouts alike).  A scheduling hint either way: same results.  (A/B runs: RWARE_PRIO=0|1, RWARE_PRIO_ROLLOUT=0|1 with RWARE_HOOKS=1 move the default only.) */
    RW_PRIO_OFF = 256,
    RW_PRIO_ON = 512,
    /* Bit-packed FLATTENED observations.  Every element of a FLATTENED observation except the two coordinates is 0.0 or 1.0
     * (rware/warehouse.py:643-673); with RW_OBS_PACKED the launches write the bits instead of 4 bytes per bit:
     *   RW_BUF_OBS_PACKED  uint32 [B][N][PW], PW = 1 + ceil(L / 32), L = rw_info.obs_length
     *     word 0                    x | y << 16 — the agent's cell indices as integers, whatever normalised_coordinates says
     *     word 1 + k / 32, bit k % 32   obs[k] != 0, for 2 <= k < L; bits 0 and 1 of word 1 (the coordinate slots) and the bits from L
     *                               upwards in the last word are 0
     * (sensor_range 1 without messages: L = 71, PW = 4 — 16 bytes per agent instead of 284).  Unpacking — obs[0] = coord(x, W), obs[1] =
     * coord(y, H) with coord the identity or, with normalised_coordinates, float32(float64(v) / float64(dim - 1)); obs[k] = float32(bit k)
     * — reproduces RW_BUF_OBS bit for bit: rw_unpack_obs on the device, rware_amd.unpack_obs in Python.
     * With the flag RW_BUF_OBS is NOT allocated (0 bytes; rw_read of it and the `obs` argument of rw_read_outputs fail with
     * RW_ERR_UNSUPPORTED); RW_BUF_FINAL_OBS (SAME_STEP autoreset) stays float32.  rw_reset, rw_refresh_obs, snapshots' restore, the fused
     * rollouts and captured graphs all produce packed rows.  FLATTENED only: the IMAGE types fail with RW_ERR_UNSUPPORTED (the
     * AGENT_DIRECTION layer holds dir + 1).  Off by default; the float32 rows stay the default and the parity path.
     * Which kernels run with it: the ahead-of-time exact-shape builds do not carry the packed rows and are never used; below 4096 envs, with
     * RW_JIT_OFF or without hipRTC the generic kernel runs (rw_info.build_kind == 0); from 4096 envs on (or with RW_JIT_FORCE) rw_create
     * compiles an exact-shape packed build through hipRTC at construction (seconds; cached on disk as described at RW_JIT_OFF; rw_info.jit
     * says which happened).  RW_PIPE_ON | RW_OBS_PACKED: the classic kernel runs and rw_jit_log() says so. */
    RW_OBS_PACKED = 1024,
    /* Per-episode return and length, kept on the device (what Gymnasium's RecordEpisodeStatistics keeps on the host; the reference has no
     * counterpart, its `info` is {}).  With RW_EPISODES_ON the engine keeps RW_BUF_EP_RETURN .. RW_BUF_EP_COUNT (below).  Per env and step,
     * in every launch form (rw_step*, tapes, fused rollouts, HIP graphs, rw_multi):
     *   - a NEXT_STEP reset step (the step that consumes the pending flag: action ignored, reward 0): running return and length become 0,
     *     nothing is recorded;
     *   - any other step: return[e][i] += reward[e][i], length[e] += 1; if the step sets `terminated`: last_return = return, last_length =
     *     length, count += 1, and afterwards return = 0, length = 0 — in all three autoreset modes (DISABLED: a caller that keeps stepping a
     *     finished env gets one record per such step; SAME_STEP: the record is taken from the terminating step, before the in-step reset);
     *   - rw_reset, masked or not: running return and length of the reset envs become 0; last_* and count are untouched.
     * rw_write seeds or zeroes all five, snapshots carry them.  Rewards are multiples of 0.5 (rware/warehouse.py:919-927, :894), so the
     * float32 sums are exact up to 2^23.  Off by default: without the flag the same kernels run and the five buffers are empty.
     * Which kernels run with it: as for RW_STATS_ON (the same compile switch carries the code) — the generic kernel below 4096 envs, with
     * RW_JIT_OFF or without hipRTC, else an exact-shape build compiled at construction; rw_jit_log says so.  Combines with RW_STATS_ON,
     * RW_OBS_PACKED, msg_bits and the IMAGE types.  RW_PIPE_ON | RW_EPISODES_ON: the classic kernel runs and rw_jit_log() says so. */
    RW_EPISODES_ON = 2048,
    /* Per-agent valid-action masks, written by the step kernels (the reference has no counterpart, its `info` is {}; JAX ports of the
     * environment ship one with every observation).  With RW_ACTION_MASK_ON the engine keeps RW_BUF_ACTION_MASK, uint8 [B][N]: one byte per
     * agent, describing the state that the observation row of the same agent describes — post-step, and post-reset for envs reset in that
     * launch.  Let t be the cell ahead of the agent along `dir`, `inside` iff t lies in the grid (Agent.req_location, rware/warehouse.py:
     * 102-112, before clamping), and `cancel` the reference's rule at :829-844: the agent carries a shelf, and the shelf layer at t is
     * non-zero, and NOT (an agent stands on t and that agent carries a shelf).  Then
     *   bit 0 (NOOP), bit 2 (LEFT), bit 3 (RIGHT)   always 1;
     *   bit 1 (FORWARD, strict)                     inside and no agent on t and not cancel;
     *   bit 4 (TOGGLE_LOAD)                         not carrying: the shelf layer under the agent is non-zero (:889-892); carrying: the
     *                                               agent's cell is not a highway (:893-895);
     *   bit 5 (FORWARD_IF_VACATED)                  inside and an agent stands on t and not cancel — the move is legal if the occupant
     *                                               leaves in the same step (a follow chain, :848-869); a permissive FORWARD mask is
     *                                               bit 1 | bit 5;
     *   bits 6, 7                                   0.
     * Operationally: bit a (a = 1..4) is set iff the reference step in which this agent requests a and every other agent requests NOOP
     * changes the agent's (x, y, dir, carrying_shelf).  With msg_bits > 0 the mask covers the Action component only.
     * Written for every env in every autoreset mode by every launch — rw_step*, tapes, HIP graphs, rw_multi, rw_reset (masked or not),
     * rw_refresh_obs, rw_snapshot_restore: a `terminated` env under DISABLED gets the mask of its final state, an env with a pending
     * NEXT_STEP reset the mask of its current state (the next step ignores its action anyway); SAME_STEP: the mask belongs to the reset
     * observation in RW_BUF_OBS, RW_BUF_FINAL_OBS gets none.  A fused rollout (rw_step_many*) leaves the mask of its LAST step.
     * Read-only (rw_write refuses it).  Off by default: without the flag the same kernels run and the buffer is empty.
     * Which kernels run with it: as for RW_STATS_ON / RW_EPISODES_ON (the same compile switch carries the code).  Combines with both, with
     * RW_OBS_PACKED, msg_bits and the IMAGE types.  RW_PIPE_ON | RW_ACTION_MASK_ON: the classic kernel runs and rw_jit_log() says so.
     * Out of scope: a per-step mask tape for rw_step_many_device (a fused rollout is open-loop — its actions exist before the launch, so
     * nothing samples from those masks; the closed-loop forms, rw_step / graphs / pipelines, get a fresh mask every step) and masks in the
     * pipelined (PIPE=1) kernels. */
    RW_ACTION_MASK_ON = 4096,
    /* uint8 IMAGE observations.  Every element of an IMAGE / IMAGE_DICT observation is an integer in 0 .. 4 (rware/warehouse.py:527-596:
     * six layers are 0 / 1, AGENT_DIRECTION holds dir + 1); with RW_OBS_IMAGE_U8 the launches write it as ONE byte instead of a float:
     *   RW_BUF_OBS  uint8 [B][N][C][2r+1][2r+1] — the same kind, the same shape, element for element (uint8) of the float the engine
     *               writes without the flag; rw_info.obs_length stays the element count per agent, the buffer holds B * N * obs_length bytes
     * (the default layer list at sensor_range 1: 45 bytes per agent instead of 180).  No unpacking step exists or is needed: a CNN's first
     * layer takes obs.float().  rw_get_buffer / rw_read / rw_write of RW_BUF_OBS and the `obs` argument of rw_read_outputs move that many
     * bytes (a float-sized rw_read fails with RW_ERR_INVALID_ARG); rw_info.obs_packed reads 2 and engine_bytes_per_env_step prices
     * N * obs_length bytes for the observation.  RW_BUF_FEATURES (IMAGE_DICT), RW_BUF_FINAL_OBS and RW_BUF_FINAL_FEATURES (SAME_STEP
     * autoreset) stay float32.  rw_step*, tapes, captured graphs, rw_multi, rw_reset (masked or not), rw_refresh_obs, snapshots' restore
     * and the fused rollouts all produce uint8 rows; the `obs_tape` of rw_step_many_device receives uint8 [T][B][N][C][2r+1][2r+1] through
     * the same pointer, at ANY byte address (a step's rows are B * N * obs_length bytes, odd for many shapes: the kernels look at the
     * address of every chunk and store 16 bytes, 4 bytes or single bytes at a time).  IMAGE and IMAGE_DICT only: FLATTENED fails with
     * RW_ERR_UNSUPPORTED (its compact format is RW_OBS_PACKED), and so do the two flags together; rw_unpack_obs and rw_debug_store_floor
     * return RW_ERR_UNSUPPORTED on such an engine.  Off by default; the float32 image stays the default and the parity path.
     * Which kernels run with it: as for RW_OBS_PACKED — the ahead-of-time exact-shape builds do not carry the uint8 rows and are never
     * used; below 4096 envs, with RW_JIT_OFF or without hipRTC the generic kernel runs (rw_info.build_kind == 0); from 4096 envs on (or with
     * RW_JIT_FORCE) rw_create compiles an exact-shape uint8 build through hipRTC at construction (rw_info.jit says which happened).
     * Combines with RW_STATS_ON, RW_EPISODES_ON, RW_ACTION_MASK_ON and msg_bits.  RW_PIPE_ON | RW_OBS_IMAGE_U8: the classic kernel runs
     * and rw_jit_log() says so. */
    RW_OBS_IMAGE_U8 = 8192,
    /* Time-limit ends reported as truncation.  The reference reports every end of an episode as `terminated` and never sets `truncated`
     * (rware/warehouse.py:935-942); a learner that bootstraps needs the two apart: reaching max_steps is no property of the state.  Per env
     * and step, after the counters are updated (:929-933), let
     *   by_inactivity = max_inactivity_steps != 0 && inactive >= max_inactivity_steps
     *   by_steps      = max_steps != 0 && steps >= max_steps
     *   done          = by_inactivity || by_steps              (the reference's `done`, unchanged)
     * Without the flag: terminated = done, truncated = 0, and RW_BUF_TRUNCATED is stored by resets only.  With RW_TIME_LIMIT_TRUNCATES, for
     * an env the launch stepped: terminated = by_inactivity, truncated = by_steps — both set when both rules fire on the same step
     * (Gymnasium's TimeLimit: truncation does not look at termination) — so terminated | truncated == done on every env and every step.
     * Everything that means "the episode ended" keeps following `done`: the pending NEXT_STEP reset, the SAME_STEP in-step reset with
     * RW_BUF_FINAL_OBS / RW_BUF_FINAL_FEATURES, the RW_EPISODES_ON record, the terminal branch of the event counters.  A NEXT_STEP reset
     * step (action ignored) writes 0 / 0; rw_reset / rw_reset_device, masked or not, clear both flags of the envs they reset and leave the
     * others alone; under RW_AUTORESET_DISABLED a finished env that keeps being stepped gets its flags by the same two rules on every
     * step.  A fused rollout leaves its last step's flags in RW_BUF_TRUNCATED, or every step's in the tape of rw_step_many_device2.
     * RW_BUF_TRUNCATED stays read-only for rw_write.  Off by default: the default is the reference's behaviour, bit for bit.
     * Which kernels run with it: as for RW_STATS_ON / RW_EPISODES_ON / RW_ACTION_MASK_ON (the same compile switch carries the code) — the
     * generic kernel below 4096 envs, with RW_JIT_OFF or without hipRTC, else an exact-shape build compiled at construction; rw_jit_log
     * says so.  Combines with every other flag, with msg_bits and the IMAGE types.  RW_PIPE_ON | RW_TIME_LIMIT_TRUNCATES: the classic
     * kernel runs and rw_jit_log() says so.  Out of scope: max_inactivity_steps as a truncation; the pipelined (PIPE=1) kernels. */
    RW_TIME_LIMIT_TRUNCATES = 16384
};

/* Device buffers (all env-major, C-contiguous).  Replaces the attributes callers read off the
 * reference object: env.grid (:302), env.agents[i].{x,y,dir,carrying_shelf,has_delivered}
 * (:82-93), env.request_queue (:263), env._cur_steps/_cur_inactive_steps (:249-250),
 * env.np_random.bit_generator.state, and the step() return tuple (:944-946). */
enum rw_buffer_kind {
    RW_BUF_OBS = 0,          /* float32 [B][N][L]  FLATTENED observation (:598-674), or, for the IMAGE
                                                   types, [B][N][C][2r+1][2r+1] (:527-596) — uint8 elements
                                                   with RW_OBS_IMAGE_U8                           */
    RW_BUF_REWARDS = 1,      /* float32 [B][N]                                                    */
    RW_BUF_TERMINATED = 2,   /* uint8   [B]        `done` (:935-941)                              */
    RW_BUF_TRUNCATED = 3,    /* uint8   [B]        always 0 (:942) — with RW_TIME_LIMIT_TRUNCATES: the step limit ended
                                                   the episode; read-only (rw_write refuses it)   */
    RW_BUF_GRID = 4,         /* int32   [B][2][H][W] layer 0 agent ids, layer 1 shelf ids (:11-14).
                                                   A DERIVED VIEW: rebuilt from the state the kernels keep (shelf
                                                   layer, agent coordinates) by rw_read / rw_get_buffer of this kind
                                                   and by rw_refresh_grid — steps enqueued after that do not touch
                                                   it (every other buffer is current after every step)           */
    /* The five agent arrays are DERIVED VIEWS as well (round 3): the kernels keep an agent as ONE packed dword
     * (cell, dir, has_delivered, carried shelf) — one load stream and one store stream per step instead of five each.
     * rw_read / rw_get_buffer of these kinds unpack the records first; rw_write of one of them re-packs all five;
     * rw_refresh_grid brings pointers borrowed earlier up to date.                                                  */
    RW_BUF_AGENT_X = 5,      /* int32   [B][N]     Agent.x (:86)                                  */
    RW_BUF_AGENT_Y = 6,      /* int32   [B][N]     Agent.y                                        */
    RW_BUF_AGENT_DIR = 7,    /* int32   [B][N]     rw_direction                                   */
    RW_BUF_AGENT_CARRY = 8,  /* int32   [B][N]     carried shelf id, 0 == none                    */
    RW_BUF_AGENT_DELIVERED = 9, /* int32 [B][N]    has_delivered                                  */
    RW_BUF_QUEUE = 10,       /* int32   [B][Q]     requested shelf ids in slot order              */
    RW_BUF_STEPS = 11,       /* int32   [B]                                                       */
    RW_BUF_INACTIVE = 12,    /* int32   [B]                                                       */
    RW_BUF_RNG = 13,         /* uint64  [6][B]     FIELD-major: state_hi, state_lo, inc_hi, inc_lo,
                                                   has_uint32, uinteger (numpy PCG64 state)       */
    RW_BUF_NEED_RESET = 14,  /* uint8   [B]        NEXT_STEP autoreset: env resets on next step   */
    RW_BUF_ACTIONS = 15,     /* int32   [B][N][1+M] staging buffer used by rw_step (host actions)  */
    RW_BUF_FEATURES = 16,    /* float32 [B][N][6]  IMAGE_DICT features: one-hot direction, on_highway,
                                                   carrying (:727-742); unused otherwise          */
    RW_BUF_AGENT_MSG = 17,   /* int32   [B][N]     bit k == message[k] of the agent (msg_bits > 0, :89)   */
    RW_BUF_FINAL_OBS = 18,   /* float32 [B][N][L]  SAME_STEP autoreset: the observation of the terminating step itself — what
                                                   Warehouse.step returns with done = True (:929-946; the image, :527-596, for the
                                                   IMAGE types) — written for the envs whose `terminated` flag that step set (rows of
                                                   other envs keep older contents); the reset observation goes to RW_BUF_OBS.  Empty in
                                                   the other autoreset modes                                              */
    RW_BUF_FINAL_FEATURES = 19, /* float32 [B][N][6] ... and, IMAGE_DICT, the feature vectors of that observation (:727-742)   */
    /* RW_STATS_ON only (empty otherwise): running totals per env since rw_create — steps add to them, NOTHING resets them (not reset(),
     * not autoreset: an episode's figure is the difference between two reads, and SAME_STEP's terminating step is counted before its
     * reset); rw_write zeroes or seeds them, snapshots carry them; int32, wrapping.  What is counted, in the reference's terms: */
    RW_BUF_STAT_DELIVERIES = 20,   /* int32 [B]  requested shelves brought to a goal: one per queue slot replaced (:907-917)             */
    RW_BUF_STAT_FAILED_MOVES = 21, /* int32 [B]  (agent, step) pairs whose FORWARD the step turned into NOOP: a loaded agent facing a
                                                 standing shelf (:836-846) or a mover that lost the collision resolution (:871-876).
                                                 A FORWARD into a wall is clamped to a self-target (:105-112) and is NOT one            */
    RW_BUF_OBS_PACKED = 22,  /* uint32  [B][N][PW] RW_OBS_PACKED only (empty otherwise; RW_BUF_OBS is empty then): the FLATTENED observation
                                                   as bits, PW = 1 + ceil(L / 32) words per agent — the format at RW_OBS_PACKED.  Read-only
                                                   (rw_write refuses it)                                                        */
    /* RW_EPISODES_ON only (empty otherwise): the semantics are at RW_EPISODES_ON.  float32 sums of multiples of 0.5: exact up to 2^23 */
    RW_BUF_EP_RETURN = 23,       /* float32 [B][N]  running return of the current episode, per agent                                      */
    RW_BUF_EP_LENGTH = 24,       /* int32   [B]     running length of the current episode                                                 */
    RW_BUF_EP_LAST_RETURN = 25,  /* float32 [B][N]  return of the env's most recently finished episode                                    */
    RW_BUF_EP_LAST_LENGTH = 26,  /* int32   [B]     its length                                                                            */
    RW_BUF_EP_COUNT = 27,        /* int32   [B]     episodes finished since rw_create (wrapping)                                          */
    RW_BUF_ACTION_MASK = 28,     /* uint8   [B][N]  RW_ACTION_MASK_ON only (empty otherwise): the valid-action byte per agent — the bits are
                                                    at RW_ACTION_MASK_ON.  Read-only (rw_write refuses it)                                */
    RW_BUF_KIND_COUNT = 29
};

/* Mirrors the constructor of rware.warehouse.Warehouse (rware/warehouse.py:146-170).  The
 * layout (`highways`, `goals`) is computed host-side exactly as _make_layout_from_params /
 * _make_layout_from_str do (:294-350) and handed over as plain arrays. */
typedef struct rw_config {
    int32_t abi_version;          /* RW_ABI_VERSION                                              */
    int32_t num_envs;             /* B                                                           */
    int32_t grid_h, grid_w;       /* grid_size (:297-300)                                        */
    int32_t n_agents;             /* N, 1..127 (more than 64: the generic kernel only)           */
    int32_t sensor_range;         /* r, 1..5 ; L = 8 + 7*(2r+1)^2 (:432-443, msg_bits == 0)      */
    int32_t request_queue_size;   /* Q                                                           */
    int32_t max_inactivity_steps; /* 0 == None                                                   */
    int32_t max_steps;            /* 0 == None                                                   */
    int32_t reward_type;          /* rw_reward_type                                              */
    int32_t normalised_coordinates;
    int32_t autoreset_mode;       /* rw_autoreset                                                */
    int32_t n_goals;
    int32_t device_id;            /* HIP device ordinal                                          */
    int32_t envs_per_workgroup;   /* 0 == engine default; otherwise a multiple of 4              */
    int32_t threads_per_workgroup;/* 0 == engine default; otherwise a multiple of 64             */
    int32_t observation_type;     /* rw_observation_type; 0 is read as FLATTENED                 */
    int32_t image_directional;    /* image_observation_directional (:167)                        */
    int32_t n_image_layers;       /* 0 == the reference default list (:160-166)                  */
    int32_t image_layers[8];      /* rw_image_layer values, channel order                        */
    int32_t msg_bits;             /* M communication bits (:152): an agent's action is then
                                     [Action, bit_0..bit_{M-1}]; FLATTENED L = 8 + (7+M)(2r+1)^2      */
    int32_t stream_flags;         /* rw_stream_flags                                              */
    const uint8_t *highways;      /* host, [H*W], 1 == highway (no shelf spawns, no unloading)   */
    const int32_t *goals_xy;      /* host, [n_goals][2] = (x, y), list order == reward order     */
    void *stream;                 /* hipStream_t to enqueue on; NULL == engine creates its own
                                     (non-blocking) stream, unless RW_STREAM_USE_GIVEN is set     */
} rw_config;

/* -- lifetime ------------------------------------------------------------------------- */
/* replaces Warehouse.__init__ (:146-292) */
int rw_create(const rw_config *cfg, rw_engine **out);
int rw_destroy(rw_engine *eng);
/* message for the most recent failing call on this engine (or on rw_create when eng == NULL) */
const char *rw_last_error(const rw_engine *eng);

/* -- the hot path ----------------------------------------------------------------------- */
/* replaces Warehouse.reset(seed, options) (:757-802).
 *   seeds: host [B] or NULL.  Non-NULL: env e is reseeded with numpy SeedSequence(seeds[e]) ->
 *          PCG64 (what gymnasium.utils.seeding.np_random does, :758-760) before the reset draws.
 *          NULL: the env's existing stream continues (reset() with seed=None).
 *   mask:  host [B] or NULL (all).  Only envs with mask[e] != 0 are reseeded/reset.
 * Observations of all envs are refreshed in RW_BUF_OBS. */
int rw_reset(rw_engine *eng, const uint64_t *seeds, const uint8_t *mask);

/* The same two operations from DEVICE arrays (no reference counterpart for the form; the semantics are Warehouse.seed / Warehouse.reset):
 *   seeds_dev: device uint64 [B], 8-byte aligned.  Env e gets the PCG64 state of numpy SeedSequence(seeds_dev[e]) — one kernel, one
 *              lane per env, the hash rw_seed_state runs on the host; has_uint32 / uinteger become 0.  rw_reset_device: or NULL — the
 *              envs' own streams continue.
 *   mask_dev:  device uint8 [B] or NULL (all).  Only envs with mask_dev[e] != 0 are reseeded / reset; every other env keeps all six
 *              RNG fields bit for bit (and, for the reset, its state).
 * Asynchrony: both calls ONLY ENQUEUE on the engine's stream — no host synchronisation, no host read of either array, no allocation.
 *   Both are therefore legal while that stream is being captured into a HIP graph, and a captured call is replayed with the graph
 *   (it then reads the arrays' contents of the replay).  The arrays must stay valid until the work has executed.
 * Results: behind the seed kernel rw_reset_device makes exactly the launch rw_reset makes (the same capture detection, the derived
 *   views marked stale), so everything rw_reset produces comes out identically: RW_BUF_OBS / RW_BUF_OBS_PACKED / uint8 rows of ALL envs
 *   refreshed, RW_BUF_ACTION_MASK, the running episode statistics of the reset envs zeroed.  rw_seed_device reseeds and nothing else
 *   (Warehouse.seed, :962-964).
 * Mask aliasing: mask_dev may be RW_BUF_TERMINATED itself — with autoreset disabled, "reset what just ended".  The reset launch rewrites
 *   that buffer, so rw_reset_device always copies the mask (asynchronous, device to device, B bytes) into a buffer of the engine's
 *   first; both kernels read the copy.
 * Errors: RW_ERR_INVALID_ARG for a NULL engine and for a seeds_dev that is not 8-byte aligned; rw_seed_device(eng, NULL, ...) too. */
/* Warehouse.seed (:962-964) for the envs with mask_dev[e] != 0 (all when NULL), from DEVICE arrays; enqueue only */
int rw_seed_device(rw_engine *eng, const uint64_t *seeds_dev, const uint8_t *mask_dev);
/* rw_reset with DEVICE arrays: uint64 [B] seeds (or NULL: the envs' own streams continue), uint8 [B] mask (or NULL: all) */
int rw_reset_device(rw_engine *eng, const uint64_t *seeds_dev, const uint8_t *mask_dev);

/* replaces Warehouse.step(actions) (:804-946) for all B envs.
 *   rw_step:        actions is a HOST array int32 [B][N] ([B][N][1+M] with msg_bits = M); copied into a
 *                   pinned staging buffer owned by the engine before the call returns (the caller may
 *                   free or overwrite its array immediately), from there to RW_BUF_ACTIONS, then launched.
 *   rw_step_device: actions is a DEVICE array of the same shape (e.g. the policy's output tensor);
 *                   no copy.  Must stay valid until the step has executed.
 * Results land in RW_BUF_OBS / REWARDS / TERMINATED / TRUNCATED. */
int rw_step(rw_engine *eng, const int32_t *actions_host);
int rw_step_device(rw_engine *eng, const int32_t *actions_dev);

/* n_steps consecutive rw_step_device launches (ONE kernel launch per step, each ordered behind the previous one on the
 * engine's stream) from a device-resident action tape int32 [tape_steps][B][N][1+M]: step k reads tape row
 * (first + k) % tape_steps.  Exactly the launches n_steps calls of rw_step_device would make, issued from one native loop:
 * replaying recorded actions, open-loop evaluation, benchmarking without per-call host overhead. */
int rw_step_tape_device(rw_engine *eng, const int32_t *tape_dev, int32_t tape_steps, int32_t first, int32_t n_steps);
/* The same launches, with two of the engine's timing events (rw_event_record slots) riding on the dispatches themselves:
 * `start_slot` takes the START timestamp of the first launch, `stop_slot` the END timestamp of the last one
 * (hipExtLaunchKernel's start / stop events) — rw_event_elapsed_ms(start_slot, stop_slot) is then the device time of the
 * n_steps launches without the two marker packets that rw_event_record would put around them (≈9 µs on a 150 µs region).
 * n_steps >= 1, start_slot != stop_slot. */
int rw_step_tape_device_timed(rw_engine *eng, const int32_t *tape_dev, int32_t tape_steps, int32_t first, int32_t n_steps,
                              int32_t start_slot, int32_t stop_slot);

/* RW_OBS_PACKED engines: the signature stays, and a non-NULL `obs_tape` receives PACKED rows — uint32 [T][B][N][PW] — through the same
 * pointer (rw_unpack_obs takes any row count, so one call unpacks a whole tape).  Any 4-byte-aligned tape works; one that starts on a
 * 16-byte boundary gets 16-byte stores.
 * RW_OBS_IMAGE_U8 engines: likewise, `obs_tape` receives uint8 [T][B][N][C][2r+1][2r+1]; a tape at any byte address works.
 * T consecutive steps from a device-resident action tape int32 [T][B][N] in ONE kernel launch: each
 * workgroup keeps its env chunk in LDS across the T steps, so per step only the actions are read and
 * obs / rewards / terminated written (rollout API; open-loop by construction —
 * the tape must exist before the launch).  Results are identical to T rw_step_device calls.  If `obs_tape` /
 * `reward_tape` / `terminated_tape` are non-NULL device pointers they receive every step's
 * outputs ([T][B][N][L] f32, [T][B][N] f32, [T][B] u8); otherwise only the last step's remain. */
int rw_step_many_device(rw_engine *eng, const int32_t *actions_dev, int32_t n_steps,
                        float *obs_tape, float *reward_tape, uint8_t *terminated_tape);
/* rw_step_many_device plus the truncated flags: `truncated_tape`, if non-NULL, is a device pointer to uint8 [T][B] and receives every
 * step's flag (RW_TIME_LIMIT_TRUNCATES; otherwise only the last step's remains, in RW_BUF_TRUNCATED).  On an engine without the flag the
 * tape is zero-filled by an asynchronous memset on the engine's stream: enqueue only, legal under stream capture. */
int rw_step_many_device2(rw_engine *eng, const int32_t *actions_dev, int32_t n_steps,
                         float *obs_tape, float *reward_tape, uint8_t *terminated_tape, uint8_t *truncated_tape);

/* One call that enqueues a step on SEVERAL engines — the shards of a single-process multi-device env (one engine per GPU).  When
 * every engine sits on a device of its own, every engine but the first is launched by a thread that rw_multi_create starts
 * (bound to that engine's device, spinning briefly between rounds, asleep otherwise), so the launches are issued side by
 * side; engines that share a device are looped over by the calling thread (their launches serialise on the device's queue
 * anyway).  rw_multi_step_device(actions_dev[k] = engine k's device action array) returns when all launches are enqueued.  Results as for rw_step_device; the engines stay usable
 * on their own between rounds (never concurrently with a round).  Destroy the rw_multi before its engines. */
typedef struct rw_multi rw_multi;
int rw_multi_create(rw_engine **engines, int32_t n, rw_multi **out);
int rw_multi_step_device(rw_multi *m, const int32_t *const *actions_dev);
int rw_multi_destroy(rw_multi *m);

/* raw device memory for action / output tapes (callers without a GPU array library) */
int rw_device_malloc(rw_engine *eng, size_t bytes, void **dev_ptr);
int rw_device_free(rw_engine *eng, void *dev_ptr);
int rw_copy_to_device(rw_engine *eng, void *dev_dst, const void *host_src, size_t bytes);
int rw_copy_to_host(rw_engine *eng, void *host_dst, const void *dev_src, size_t bytes);

/* bring the derived views — RW_BUF_GRID and RW_BUF_AGENT_X .. RW_BUF_AGENT_DELIVERED — up to date with the steps enqueued so
 * far (three small kernels on the engine's stream; a no-op when nothing ran since the last refresh).  For callers that
 * hold a borrowed pointer / a zero-copy tensor of one of them. */
int rw_refresh_grid(rw_engine *eng);
/* Move the engine to another stream (a hipStream_t; NULL = the device's default stream): later calls enqueue there.  Work
 * already enqueued stays where it is — ordering the two streams is the caller's business (events).  An engine-owned stream is
 * drained and destroyed.  For callers that set up stream capture after the engine exists (WarehouseVecEnv.capture_loop). */
int rw_set_stream(rw_engine *eng, void *stream);
/* Tell the engine that steps ran which its host side did not see — a HIP graph holding rw_step_device launches was replayed
 * (replays run without host code) — so that the next rw_read / rw_get_buffer / rw_write of a derived view rebuilds it.  The
 * engine also notices by itself when one of its launches is being captured (hipStreamIsCapturing) and from then on rebuilds
 * the derived views on every request; this call is for graphs captured by other means. */
int rw_mark_views_stale(rw_engine *eng);

/* recompute RW_BUF_OBS (RW_OBS_PACKED: RW_BUF_OBS_PACKED; RW_OBS_IMAGE_U8: as uint8) from the current state (after rw_write of state buffers) */
int rw_refresh_obs(rw_engine *eng);
/* packed rows -> float32 rows on the device (no reference counterpart): `packed_dev` uint32 [n_rows][PW], `obs_f32_dev` float32
 * [n_rows][L], both device pointers, one row per (env, agent) — RW_BUF_OBS_PACKED itself (n_rows = B * N), a slice of it, or a
 * [T][B][N][PW] tape of rw_step_many_device (n_rows = T * B * N).  Enqueued on the engine's stream; the shape facts (L, PW, grid size,
 * normalised_coordinates) are the engine's.  The result equals what RW_BUF_OBS would hold, bit for bit.  Any FLATTENED engine, with or
 * without RW_OBS_PACKED. */
int rw_unpack_obs(rw_engine *eng, const uint32_t *packed_dev, float *obs_f32_dev, int64_t n_rows);

/* -- gather and unpack packed minibatches on the device, into float32 / float16 / bfloat16: rw_unpack_obs_gather ---------------- */
/* (declared in a header of its own, which this one pulls in: a caller includes rware_hip.h and has it) */
#include "rware_hip_minibatch.h"

/* Warehouse.get_global_image (:966-1040) for all B envs, from the engine's current state, into a DEVICE array of the caller's — the
 * global-state input of a centralised critic, without a host visit.
 *   layers:       n_layers values of rw_image_layer (1 .. 8, duplicates allowed), copied by value at the call
 *   pad_to_shape: NULL, or {C', H', W'} with C' >= n_layers, H' >= grid_h, W' >= grid_w; zero padding split as :1029-1033
 *                 (before = d / 2, after = d - d / 2, on all three axes)
 *   elem:         0 float32, 1 uint8 (every element is an integer in 0 .. 4)
 *   out_dev:      [B][C'][H'][W'] of that element type, any alignment of the element type; every element is written, the padding
 *                 zeros included, and nothing else
 * Layers: SHELVES, AGENTS, GOALS 0 / 1; ACCESSIBLE 1 except under an agent; REQUESTS 1 at the cells of the queued shelves (a carried
 * requested shelf lies under its carrier); AGENT_DIRECTION (dir + 1) and AGENT_LOAD (1 for an agent that carries a shelf) are written as
 * the reference writes them, `layer[ag.x, ag.y]` on an (H, W) array (:1003, :1008): on the mirrored cell, the highest agent index winning
 * a shared one.  Where the reference raises IndexError there (x >= grid_h or y >= grid_w; AGENT_LOAD: of a carrying agent) that agent
 * writes nothing and the next rw_sync returns RW_ERR_INDEX, as for the IMAGE observations.
 * Asynchrony: the call ONLY ENQUEUES one kernel on the engine's stream — no host synchronisation, no allocation, no host-to-device copy
 *   (the layer list and the shape travel in the kernel's arguments), no derived view is refreshed: the kernel reads the shelf layer, the
 *   packed agent records and the queue as the step kernels keep them.  It is therefore legal while that stream is being captured into a
 *   HIP graph and is replayed with the graph.  The image describes the state RW_BUF_OBS describes at that point of the stream (after a
 *   SAME_STEP autoreset the reset state, after a NEXT_STEP termination the terminal state).  Any engine: every observation type and flag.
 * Errors: RW_ERR_INVALID_ARG for a NULL engine / layers / out_dev, n_layers outside 1 .. 8, a layer outside 0 .. 6, a pad dimension
 *   smaller than the image, elem other than 0 / 1, a float32 out_dev that is not 4-byte aligned, and for an image of more than 2^30
 *   elements per env ("slice it": smaller padding, or fewer layers per call). */
int rw_global_image(rw_engine *eng, const int32_t *layers, int32_t n_layers, const int32_t *pad_to_shape, int32_t elem, void *out_dev);

/* -- the global state as byte records, and minibatches of images gathered from them: rw_global_records, rw_global_image_gather --- */
/* (declared in a header of its own, which this one pulls in: a caller includes rware_hip.h and has it) */
#include "rware_hip_global_state.h"

/* -- GAE(lambda) advantages and returns from the rollout's reward, flag and value tapes, in one launch ---------------------------- */
/* (declared in a header of its own, which this one pulls in: a caller includes rware_hip.h and has it) */
#include "rware_hip_advantages.h"

/* wait for everything enqueued; returns RW_ERR_INVALID_ACTION if any step since the last
 * rw_sync saw an out-of-range action (that action was executed as NOOP), else RW_OK */
int rw_sync(rw_engine *eng);

/* -- buffers ---------------------------------------------------------------------------- */
int rw_get_buffer(rw_engine *eng, int kind, void **dev_ptr, size_t *bytes);
/* synchronous copies between a buffer and host memory (state inspection / injection) */
int rw_read(rw_engine *eng, int kind, void *host_dst, size_t bytes);
/* the step() return tuple (:944-946) to host memory in one round trip: RW_BUF_OBS / REWARDS / TERMINATED (/ FEATURES) copied
 * back to back, one synchronisation; any pointer may be NULL (skipped).  `truncated` is always False (:942): nothing to read.
 * (RW_OBS_IMAGE_U8: `obs` receives the buffer's B * N * obs_length BYTES through the same pointer.) */
int rw_read_outputs(rw_engine *eng, float *obs, float *rewards, uint8_t *terminated, float *features);
/* rw_read_outputs plus RW_BUF_TRUNCATED (B bytes; all 0 without RW_TIME_LIMIT_TRUNCATES), still one synchronisation */
int rw_read_outputs2(rw_engine *eng, float *obs, float *rewards, uint8_t *terminated, uint8_t *truncated, float *features);
int rw_write(rw_engine *eng, int kind, const void *host_src, size_t bytes);
/* rebuild RW_BUF_GRID exactly like Warehouse._recalc_grid (:749-755) from explicit shelf
 * positions (host int32 [B][S][2] = (x,y) per shelf id; later ids overwrite earlier) and the
 * current agent positions.  This is how the reference's own tests inject state. */
int rw_recalc_grid(rw_engine *eng, const int32_t *shelf_xy, int32_t n_shelves);

/* -- snapshot / restore (checkpointing the batched env state) ------------ */
/* A snapshot is a device-resident copy of everything reset()/step() evolve: shelf layer, packed agent
 * records, queue, counters, PCG64 streams, pending-autoreset flags (the int32 views are derived from these).  Saving and restoring are device-to-
 * device copies on the engine's stream (tens of microseconds); restore also refreshes RW_BUF_OBS, so
 * the engine continues bit-identically from the saved point. */
typedef struct rw_snapshot rw_snapshot;
int rw_snapshot_create(rw_engine *eng, rw_snapshot **out);
int rw_snapshot_save(rw_engine *eng, rw_snapshot *snap);
int rw_snapshot_restore(rw_engine *eng, const rw_snapshot *snap);
int rw_snapshot_destroy(rw_engine *eng, rw_snapshot *snap);

/* -- restore or clone single envs from a snapshot, by index, on the device: rw_snapshot_restore_indexed ----------------------- */
/* (declared in a header of its own, which this one pulls in: a caller includes rware_hip.h and has it) */
#include "rware_hip_restore.h"

/* -- introspection ---------------------------------------------------------------------- */
typedef struct rw_info {
    int32_t num_envs, grid_h, grid_w, n_agents, request_queue_size, n_shelves, obs_length;
    int32_t envs_per_workgroup, threads_per_workgroup, n_workgroups, lds_bytes;   /* of the per-step launches; the fused rollout may run on another
                             build of the same shape (13 .. 16 agents: per-step launches on 4-env workgroups below one round of workgroups and
                             between one and four, rollouts on 8-env ones; 17 .. 19 agents below 8192 envs likewise; rw_create's measured rule) */
    int32_t device_id, compute_units;
    int32_t specialised;  /* 1: a kernel build with this task's shapes folded in at compile time is in use */
    int32_t wave_priority; /* bit 0: the per-step launches raise their wavefronts' priority (s_setprio 3) from the start of the kernel to
                             the barrier behind the agent phases, so that the dependent chain in front of the first observation store is
                             not queued behind the neighbours' store phase on the same CU; bit 1: the fused rollouts do (every step of the
                             launch).  rw_create's measured rule: on while a step's observations stay under 200 MB (past that nothing moves),
                             except for the per-step launches of 13 .. 16 agents at sensor_range 1 on 8-env workgroups beyond half a round
                             of workgroups (on their 4-env workgroups, and up to half a round of 8-env ones, it is on) (A/B runs:
                             RWARE_PRIO=0|1, RWARE_PRIO_ROLLOUT=0|1 with RWARE_HOOKS=1).  A scheduling hint, never a different result.
                             (The slot was `state_layout`, 0 since round 3.) */
    int32_t build_kind;   /* which build of the step kernel runs: 0 generic (every shape at run time), 1 exact-shape, 2 agent-count-
                             static (shapes + agent count folded in, request-queue length at run time), 3 size-static (grid folded in,
                             agent count and queue length at run time).  (Occupies what was alignment padding: same struct size.) */
    int64_t algorithmic_bytes_per_env_step; /* SURVEY.md §8(d) formula                           */
    char device_name[128];
    char arch_name[64];
    int32_t obs_stores_stream; /* 1: the per-step kernel stores the observation stream with the non-temporal hint
                                  (rw_stream_flags); the fused rollout kernel (rw_step_many_device) always stores cached */
    int32_t jit;               /* 0: an ahead-of-time build runs; 1: an exact-shape build compiled by this rw_create (hipRTC); 2: the
                                  same, read from the disk cache; -1: run-time specialisation was tried and is not in use (rw_jit_log) */
    int64_t engine_bytes_per_env_step; /* bytes this engine's state layout has to move per env-step: shelf shadow (1 or 2 B per
                                  cell) + packed agent records r/w + actions + queue + counters / flags + observation + rewards +
                                  terminated (+ messages r/w, IMAGE_DICT features; RW_EPISODES_ON: running return and length r/w; RW_ACTION_MASK_ON: N bytes; RW_TIME_LIMIT_TRUNCATES: truncated, 1 byte).  The PMC traffic of a step is checked against
                                  it; bench.py prices `frac_engine` on it (<= 1 by construction)                               */
    int32_t stagger_ticks;     /* > 0: the k-th of the first eight workgroups a CU receives starts k * stagger_ticks * 10 ns late, so that
                                  the workgroups of a CU do not run their load / agent / store phases in lock-step.  rw_create's measured rule,
                                  in rounds of the per-step launches' workgroups: 13 .. 16 agents at sensor_range 1 on 8-env workgroups —
                                  550 ns from half a round to one round and from four rounds on; launches that do NOT run at raised wavefront
                                  priority (wave_priority bit 0 clear: steps of >= 200 MB of observations) — <= 12 agents 250 ns from two
                                  rounds on, 13 .. 16 agents at sensor_range 2 400 ns up to two rounds; else 0: with the priority the delay is
                                  only a delay (A/B runs: RWARE_STAGGER_TICKS=n with RWARE_HOOKS=1; 0 = off).  The fused rollouts carry the
                                  same value.  A delay, never a different result */
    int32_t pipe_envs_per_workgroup; /* != 0: rw_step* launches run the chunk-pipelined persistent build with chunks of this many envs ... */
    int32_t pipe_workgroups;         /* ... on this many persistent workgroups (rw_stream_flags RW_PIPE_ON / RW_PIPE_OFF)              */
    int32_t stats;                   /* a bit set: bit 0 RW_STATS_ON — RW_BUF_STAT_* are kept; bit 1 RW_EPISODES_ON — RW_BUF_EP_* are kept; bit 2 RW_ACTION_MASK_ON — RW_BUF_ACTION_MASK is written; bit 3 RW_TIME_LIMIT_TRUNCATES — RW_BUF_TRUNCATED is live
                                        (an engine with only RW_STATS_ON reads 1, as before; was `reserved[1]`: same struct size)      */
    int32_t obs_packed;              /* 1: RW_OBS_PACKED — the launches write RW_BUF_OBS_PACKED, RW_BUF_OBS is empty; engine_bytes_per_env_step
                                        prices the packed row (appended with ABI 4).  2: RW_OBS_IMAGE_U8 — the elements of RW_BUF_OBS are
                                        uint8; engine_bytes_per_env_step prices obs_length bytes per agent                           */
} rw_info;
int rw_get_info(const rw_engine *eng, rw_info *out);
/* what the run-time specialisation did for this engine: cache file / compile time, or why it is not in use ("" if not tried) */
const char *rw_jit_log(const rw_engine *eng);
/* the compile half of the run-time specialisation, without a device (build checks, cache warm-up on a login node): `shape` =
 * {sensor_range, H, W, N, Q, S, envs per workgroup, 256, msg_bits, wide shelf ids, observation kind (0 FLATTENED, 1 IMAGE,
 * 2 FLATTENED + messages, 3 IMAGE + messages), baked image layers, packed layer list, image_directional (-1 for FLATTENED), non-temporal stores,
 * packed observation rows (1: the build of an RW_OBS_PACKED engine — with an IMAGE kind: of an RW_OBS_IMAGE_U8 engine)};
 * returns the size of the gfx code object (compiled or found in the disk cache), -1 on failure (`log` says why). */
int64_t rw_jit_probe(const int32_t shape[16], const char *arch, char *log, size_t log_len);

/* On-device self-test (no engine needed; no reference counterpart — the reference is CPU Python): runs, on HIP device `device_id`,
 * the two toolchain / hardware facts the step kernels are written around — cross-lane exchange results compared as values in
 * registers of their own (a DPP move folded into a non-commutative instruction came out with swapped operands on gfx950), and an
 * LDS-DMA stage-in that is waited for explicitly in front of the workgroup barrier (a run-time compiled build once left it in flight)
 * — with code compiled into this library, so it runs where there is no hipcc.  RW_OK, or RW_ERR_SELFTEST with the counts in `log`.
 * RWARE_SELFTEST_BREAK=1 (with RWARE_HOOKS=1) runs the known-bad forms instead (tests: the guard has to be able to fail). */
int rw_selftest(int32_t device_id, char *log, size_t log_len);

/* numpy SeedSequence(seed) -> PCG64 initial state, as 6 uint64 in RW_BUF_RNG field order.
 * Pure host function (exposed so tests can check the seeding against numpy). */
int rw_seed_state(uint64_t seed, uint64_t out[6]);

/* -- timing on the engine's own stream (hipEvents), used by bench.py --------------------- */
int rw_event_record(rw_engine *eng, int32_t slot /* 0..7 */);
int rw_event_elapsed_ms(rw_engine *eng, int32_t slot_begin, int32_t slot_end, float *ms);

/* measurement aid (no reference counterpart): `n_launches` back-to-back launches of a kernel that only WRITES one step's
 * observations — the engine's launch geometry and store instruction, nothing else — timed with HIP events on the first / last launch:
 * the least any kernel producing this step's observations can take on this device (bench.py reports it beside the 8 TB/s roofline).
 * RW_BUF_OBS is refreshed afterwards (rw_refresh_obs).  Uses the engine's timing-event slots 6 and 7 (rw_event_record).
 * RW_ERR_UNSUPPORTED on an RW_OBS_IMAGE_U8 engine (the store-only kernel writes dword rows). */
int rw_debug_store_floor(rw_engine *eng, int32_t n_launches, float *ms_per_launch);

/* profiling aid: runs ONE step (device actions) with per-workgroup phase stamps taken from the
 * 100 MHz wall clock; host_out receives uint64 [n_workgroups][n_marks].  Call with host_out ==
 * NULL to query the two sizes first. */
int rw_debug_timeline(rw_engine *eng, const int32_t *actions_dev, uint64_t *host_out,
                      int32_t *n_workgroups, int32_t *n_marks);

int rw_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RWARE_HIP_H */
