/* rware_hip_advantages.h — part of the C-ABI of include/rware_hip.h, which includes this file: GAE(lambda) advantages and returns from a
 * rollout's reward, flag and value tapes, in one launch.  Do not include it on its own: it needs rw_engine, and sits inside rware_hip.h's
 * extern "C". */
#ifndef RWARE_HIP_ADVANTAGES_H
#define RWARE_HIP_ADVANTAGES_H
#ifndef RWARE_HIP_H
#error "include rware_hip.h, which includes this header"
#endif

/* -- advantages and returns from the rollout tapes on the device ---------------------------------- */
/* T = n_steps, B = n_envs, N = n_agents, K = n_heads value heads per env: K == N a per-agent critic, K == 1 one value per env (a
 * centralised critic on the team reward).  All arrays are C-contiguous DEVICE arrays; only the kernel reads or writes them.
 *   rewards_dev       float32 [T][B][N]   the rollout's reward tape
 *   values_dev        float32 [T][B][K]   V of the observation step t acted on
 *   last_values_dev   float32 [B][K]      V of the observation after step T-1
 *   terminated_dev    uint8   [T][B]      non-zero: set
 *   truncated_dev     uint8   [T][B]      or NULL: all zero
 *   final_values_dev  float32 [T][B][K]   or NULL: V(final_obs); read only where truncated && !terminated, and only WITHOUT
 *                                         RW_GAE_NEXT_STEP — with that flag the pointer is ignored (it is not even looked at)
 *   prev_ended_dev    uint8   [B]         or NULL (no): whether the step before this tape ended an episode, terminated | truncated of
 *                                         the previous tape's last row; read only WITH RW_GAE_NEXT_STEP — without it the pointer is ignored
 *   advantages_dev    float32 [T][B][K]   output
 *   returns_dev       float32 [T][B][K]   output, or NULL
 *   valid_dev         uint8   [T][B]      output, or NULL: 0 on a reset step, else 1
 * flags: RW_GAE_NEXT_STEP — the tape was written under RW_AUTORESET_NEXT_STEP: the step after an episode end is a reset step (reward 0,
 *   no flags, its observation the terminal one), so values[t+1] is already V(final obs), the bootstrap of a truncated end, and the reset
 *   step itself is no transition.  Without it (SAME_STEP, or DISABLED with a masked reset inside the loop) obs[t+1] is the new episode's
 *   first observation: a truncated end bootstraps from final_values, or from 0 without them.
 *   RW_GAE_TEAM_REWARD — every head sees the env's summed reward; required when K == 1 and N > 1.
 * Per column (b, k), backwards in time, every operation a separately rounded float32 operation in exactly this order (nothing is
 * contracted into a fused multiply-add), g = gamma, gl = (float)(gamma * lam) — one float32 multiply on the host:
 *   carry = 0; next_v = last_values[b][k]
 *   for t = T-1 .. 0:
 *     r     = TEAM ? ((rewards[t][b][0] + rewards[t][b][1]) + ...) + rewards[t][b][N-1] : rewards[t][b][k]
 *     v     = values[t][b][k]
 *     term  = terminated[t][b] != 0;  trunc = truncated && truncated[t][b] != 0
 *     reset = NEXT_STEP && (t > 0 ? (terminated[t-1][b] | truncated[t-1][b]) != 0 : prev_ended && prev_ended[b] != 0)
 *     boot  = term ? 0 : trunc ? (NEXT_STEP ? next_v : final_values ? final_values[t][b][k] : 0) : next_v
 *     delta = (r + g * boot) - v
 *     adv   = (term || trunc) ? delta : delta + gl * carry
 *     if reset: adv = 0                        (takes precedence over the flags of step t)
 *     advantages[t][b][k] = adv;  returns[t][b][k] = adv + v;  valid[t][b] = !reset
 *     carry = adv;  next_v = v
 * NaN and infinity propagate as IEEE says.  returns on a reset step is values[t]: an unmasked value loss sees zero error there.
 * The engine supplies the device and the stream only: B and N are the tape's and need not be the engine's (another shard's tape, a
 * concatenation), and every observation type and flag set is accepted.
 * Asynchrony: exactly one kernel launch on the engine's stream — no host synchronisation, no allocation, no host-to-device copy; legal
 *   while the stream is being captured and replayed with the graph (a replay reads the arrays' contents at replay time).  All arrays
 *   must stay valid until the work has run.  Large tapes (from 262 144 columns B*K on, no team reward) whose float arrays all start on
 *   16-byte boundaries, with B*K a multiple of 4, are read and written 16 bytes at a time; any others element by element, with the
 *   same values.
 * Errors: RW_ERR_INVALID_ARG, rw_last_error naming the argument, for a NULL engine, a NULL args or a NULL required pointer; n_steps,
 *   n_envs, n_agents or n_heads below 0; n_heads neither 1 nor n_agents; n_heads == 1 with n_agents > 1 and no RW_GAE_TEAM_REWARD;
 *   unknown flag bits or reserved != 0; gamma or lam not finite or outside [0, 1]; a float pointer that is not 4-byte aligned; an
 *   output whose bytes overlap an input's or another output's; more columns (B*K, B*N >= 2^31) or elements (T*B*max(N, K) >= 2^40) than
 *   one launch holds: compute in slices of envs.  n_steps == 0 or n_envs == 0 is RW_OK and writes nothing. */
enum rw_gae_flags { RW_GAE_NEXT_STEP = 1, RW_GAE_TEAM_REWARD = 2 };
typedef struct rw_gae_args {
    const float *rewards_dev, *values_dev, *last_values_dev;
    const uint8_t *terminated_dev, *truncated_dev;      /* truncated_dev may be NULL */
    const float *final_values_dev;                      /* may be NULL */
    const uint8_t *prev_ended_dev;                      /* may be NULL */
    float *advantages_dev, *returns_dev;                /* returns_dev may be NULL */
    uint8_t *valid_dev;                                 /* may be NULL */
    int32_t n_steps, n_envs, n_agents, n_heads;         /* T, B, N, K */
    float gamma, lam;
    int32_t flags, reserved;                            /* reserved: 0 */
} rw_gae_args;
int rw_gae(rw_engine *eng, const rw_gae_args *args);

#endif /* RWARE_HIP_ADVANTAGES_H */
