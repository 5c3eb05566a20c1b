/*
 * mgx.h -- C ABI of the MI355X-native batched MultiGrid step/observation engine (libmgx.so).
 *
 * The reference (ini/multigrid) is pure Python and has no FFI of its own: the seam this
 * library replaces is the pair of Python call sites
 *     multigrid/base.py:361-366   image = gen_obs_grid_encoding(grid.state, agent_states, view_size, see_through_walls)
 *     multigrid/base.py:333-340   step_count += 1; rewards = handle_actions(actions); gen_obs(); terminations; truncated
 * batched over B independent environments.  Every entry point takes plain device pointers and sizes, returns 0 or
 * a negative MGX_ERR_* code, never throws, never allocates, never frees and never retains a pointer.  All work is
 * enqueued on the HIP stream passed by the caller (a hipStream_t cast to void*; NULL = the default stream); the
 * functions do not synchronise.
 *
 * Tensor layouts (all contiguous, device memory):
 *   grid        u16[B, H, W]      PACKED cells (MgxCell): cell (x, y) of env b at (b*H + y)*W + x -- the [y][x] transpose of
 *                                 the reference's Grid.state (W,H,3) (multigrid/core/grid.py:54), each (type, color, state)
 *                                 triple in 16 bits:
 *                                     [3:0] type   [10:8] color   [13:12] state   [15] opaque
 *                                     [6:4] + {[7], [11], [14]}: what a BOX holds (ABI 9, below); zero on every other cell
 *                                 opaque = 1 for a cell one cannot see through (multigrid/utils/obs.py:46-63: a wall, or a door
 *                                 that is not open); it is part of the format (the kernels keep it up to date on every cell
 *                                 they write).  Two bytes per cell instead of the reference's three int64: a third less grid
 *                                 traffic and aligned 16-bit cell accesses on the device.  mgx_pack_grid / mgx_unpack_grid
 *                                 convert from / to u8[B,H,W,3] (type, color, state) bytes on the device; values the 16 bits
 *                                 cannot hold (type > 15, color > 7, state > 3 -- the reference has types 0-10, colors 0-5,
 *                                 states 0-2 and directions 0-3) are reported by mgx_pack_grid.
 *                                 BOX CONTENTS (ABI 9).  A box may hold an object (multigrid/core/world_object.py:574-605:
 *                                 Box(color, contains); Box.toggle replaces the box by its content).  Neither Grid.state nor an
 *                                 observation shows it, so it rides in bits the triple leaves free: in the (type, color, state)
 *                                 BYTES (mgx_pack_grid* input, mgx_unpack_grid output, an agent row's carried cell) the state
 *                                 byte of a box is  state | kind << 2 | content colour << 5,  kind = 0 nothing, 1 key, 2 ball,
 *                                 3 goal, 4 floor, 5 lava, 6 wall, 7 door (closed and unlocked, as Door(color) constructs it);
 *                                 in the packed cell: kind in [6:4], colour in {[7], [11], [14]}.  The kernels carry it through
 *                                 pickup / drop and put the content on the grid when the box is toggled; observations and
 *                                 mgx_full_obs show the box as (box, color, 0) whatever it holds.  A box in a box and doors in
 *                                 other states are not representable (the host refuses them: multigrid_amd.world.Box).
 *                                 PRECONDITION: the outer ring of cells (x = 0, x = W-1, y = 0, y = H-1) of every env is the
 *                                 reference's WALL = (wall, grey, 0) (multigrid/utils/obs.py:14).  Every env of the reference
 *                                 starts from Grid.wall_rect(0, 0, W, H) (multigrid/core/grid.py:183-218; envs/empty.py:158,
 *                                 core/roomgrid.py:203-218) and no action can change a wall, so it holds for every reachable
 *                                 state.  The kernels use it twice: a front cell outside the grid never has to be tested
 *                                 (the agent cannot stand on the ring), and a view cell outside the grid -- which
 *                                 obs.py:199-202 shows as WALL -- is read from the ring cell next to it (the gather clamps its
 *                                 coordinates instead of carrying an in-bounds mask per view).  The host side checks it on
 *                                 import (multigrid_amd/layouts.py: check_walled).
 *   agents      u8 [B, A, 8]      packed AgentState row (multigrid/core/agent.py:222-232, 72 B -> 8 B):
 *                                 [0]=color [1]=dir [2]=x [3]=y [4]=terminated [5]=carry.type [6]=carry.color
 *                                 [7]=carry.state (a carried box: | its content << 2, see "grid") ; "carrying nothing" = the
 *                                 empty cell (1,0,0) (agent.py:337-346).
 *   rng         u64[B, 4]         per-env numpy PCG64 state of `env.np_random`: [state_lo, state_hi, inc_lo, inc_hi].
 *                                 Advanced by A draws per step when A > 1 (multigrid/base.py:396-399).
 *   step_count  i32[B]            multigrid/base.py:292, 333
 *   actions     i8 [B, A]         multigrid/core/actions.py:5-15 (0..6); -1 = agent absent from the actions dict
 *                                 (multigrid/base.py:403-404); any other value = MGX_ERR_UNKNOWN_ACTION (base.py:473).
 *   aux         u8 [B, 16]        the env subclass' own attributes that its step() hook uses (in/out; may be NULL for
 *                                 MGX_KIND_EMPTY):
 *                                   BlockedUnlockPickup  [0..2] = encoding of the target box `self.obj`
 *                                                        (multigrid/envs/blockedunlockpickup.py:147, 172)
 *                                   RedBlueDoors         [0,1] = blue door (x,y), [2,3] = red door (x,y)
 *                                                        (multigrid/envs/redbluedoors.py:158-168); [4] = 1 while the blue
 *                                                        Door OBJECT is closed although Grid.state (= `grid`) still says
 *                                                        open: the hook closes it without grid.update
 *                                                        (redbluedoors.py:185).  The rules act on the object, obs on
 *                                                        `grid`; updated by the step
 *                                   LockedHallway        [0] = number of doors, [1] = bit k set once door k is in
 *                                                        `self.unlocked_doors` (updated by the step), [2+2k, 3+2k] =
 *                                                        door k (x,y), [15] = 1 when the last step reported every agent
 *                                                        terminated (multigrid/envs/locked_hallway.py:203-227)
 *                                                        With more than 6 rooms: [0] = 0x80 | number of doors (<= 16),
 *                                                        [1], [2] = unlocked mask (16 bits), [3] = room_size, [4] =
 *                                                        len(self.rooms) (rooms are keyed by door colour: repeated
 *                                                        colours count once, and that count ends the episode); door k =
 *                                                        (row k/2, side k%2) sits mid-wall at x = side ? 2(rs-1) : rs-1,
 *                                                        y = row (rs-1) + (rs-1)/2 (add_door(..., rand_pos=False):
 *                                                        (top + bottom) // 2, multigrid/core/roomgrid.py:108)

 *   obs         u8 [B, A, v, v, 3] image[i][j][c] exactly as multigrid/utils/obs.py:65-102 returns it
 *   dir         u8 [B, A]         obs['direction'] (multigrid/base.py:359, 372)
 *   reward      f64[B, A]         multigrid/base.py:393, 503-507, 598-602 (bit-identical Python float arithmetic)
 *   terminated  u8 [B, A]         multigrid/base.py:338 (+ env hook)
 *   truncated   u8 [B]            multigrid/base.py:339-340
 *   err         i32[2]            err[0] += number of envs that met an unknown action; err[1] = min such env index.
 *                                 The caller initialises it to {0, INT32_MAX} and inspects it after synchronising.
 */
#ifndef MGX_H
#define MGX_H

#if !defined(__HIPCC_RTC__)      /* (hipRTC has the fixed-width integer types built in and no system headers) */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_ABI_VERSION 11

enum {
    MGX_OK = 0,
    MGX_ERR_INVALID_ARGUMENT = -1, /* NULL pointer, bad spec (even / <3 view size: multigrid/core/agent.py:78-79) */
    MGX_ERR_UNKNOWN_ACTION = -2,   /* reported through `err`, mirrors ValueError at multigrid/base.py:473-474 */
    MGX_ERR_UNSUPPORTED = -3,      /* spec outside the compiled limits (MGX_MAX_AGENTS, MGX_MAX_VIEW, LDS budget) */
    MGX_ERR_LAUNCH = -4            /* hipLaunchKernel failed; see mgx_last_hip_error() */
};

enum { MGX_KIND_EMPTY = 0, MGX_KIND_BLOCKEDUNLOCKPICKUP = 1, MGX_KIND_REDBLUEDOORS = 2, MGX_KIND_LOCKEDHALLWAY = 3,
       MGX_KIND_RULES = 4 };     /* ABI 9: a declarative step() hook, see MgxHookRule */

/* (ABI 9) MGX_KIND_RULES: the step() post-hook of a USER-DEFINED env, declared instead of compiled in.  The reference's envs
 * end their episodes in a `step` override that runs after the base step: `if agent.state.carrying == self.obj:
 * self.on_success(...)` (multigrid/envs/blockedunlockpickup.py:166-175), `if action == toggle and fwd_obj == self.blue_door ...:
 * self.on_failure(...)` (multigrid/envs/redbluedoors.py:170-187).  Both shapes as a table in the env's `aux`:
 *     aux[0] = n, the number of rules (<= MGX_MAX_RULES); rule k = the five bytes aux[1 + 5k ..]: { op, a, b, effect, cond }
 *       op      MGX_RULE_CARRIES    an agent carries an object of type a and colour b   (`agent.state.carrying == self.obj`)
 *               MGX_RULE_TOGGLES_AT an agent's action this step was `toggle` and the cell in front of it is (x, y) = (a, b)
 *                                   (`fwd_obj == self.door` for an object that does not move)
 *       effect  MGX_EFFECT_SUCCESS  on_success(agent): terminated (mode 'any': every agent), reward (multigrid/base.py:478-507)
 *               MGX_EFFECT_FAILURE  on_failure(agent)                                        (multigrid/base.py:509-532)
 *       cond    TOGGLES_AT only: MGX_COND_ALWAYS, MGX_COND_DOOR_OPEN / MGX_COND_DOOR_SHUT = only while the cell at (x, y) holds a
 *               door that is open / not open AFTER the step (`self.door.is_open`)
 * Evaluated after the base step on the post-step state, rule by rule in table order; within a CARRIES rule the agents in index
 * order (`for agent in self.agents`), within a TOGGLES_AT rule in `hook_order` (`for agent_id, action in actions.items()`).  As with
 * the compiled hooks the observation of the step is rendered BEFORE the hook; `terminated` / `reward` reflect it.  BlockedUnlockPickup
 * is the one-rule table { CARRIES, box, colour, SUCCESS } (tests/test_rule_hooks.py holds it against the compiled kind). */
#define MGX_MAX_RULES 3
enum { MGX_RULE_CARRIES = 1, MGX_RULE_TOGGLES_AT = 2 };
enum { MGX_EFFECT_SUCCESS = 1, MGX_EFFECT_FAILURE = 2 };
enum { MGX_COND_ALWAYS = 0, MGX_COND_DOOR_OPEN = 1, MGX_COND_DOOR_SHUT = 2 };

#define MGX_AUX_BYTES 16

typedef uint16_t MgxCell;        /* packed grid cell, see "grid" above */
#define MGX_CELL_BYTES 2

/* (ABI 9) COMPACT cells: the grid as ONE byte per cell, for large grids -- MgxSpec.cell_bytes = 1.  A step streams an env's whole
 * grid for its agents' views, so on a 64x64 grid (BASELINE.json configs[4]) the grid is half of all the bytes the step moves and
 * its LDS tile decides how many envs a wavefront can own: at one byte per cell the traffic falls by a third and a wavefront
 * steps two such envs instead of one.  A (type, color, state) triple holds 4 + 3 + 2 bits, but only doors (state) and the agent
 * overlay (direction) use the third field, so type and state are coded JOINTLY:
 *     [3:0] tcode   0..10 = the reference's type index with state 0 (4 = an OPEN door, 10 = an agent facing right);
 *                   11 = closed door, 12 = locked door; 13, 14, 15 = agent facing down / left / up
 *     [6:4] color   [7] opaque (as in MgxCell: a wall, or a door that is not open)
 * WALL = (wall, grey, 0) is 0xD2.  Wherever this header says `MgxCell *grid` (grid, pool_grid) an engine whose spec has
 * cell_bytes = 1 takes MgxCell8[B,H,W] through the same parameter (cast).  Served in this format: mgx_gen_obs, mgx_step,
 * mgx_step_autoreset, mgx_step_ex (steps = 1, no one_hot, no generate), mgx_step_chains / mgx_sub_shards, mgx_reset_done,
 * mgx_full_obs, mgx_check_grid, mgx_launch_info and the conversions mgx_pack_grid8_env / mgx_unpack_grid8; every other entry
 * point returns MGX_ERR_UNSUPPORTED for such a spec (rollouts, one-hot output, device-side generation and persistent stepping
 * keep the 16-bit cells).  Same results bit for bit in either format (tests/test_compact_cells.py). */
typedef uint8_t MgxCell8;

/* (ABI 9) BYTE grids: MgxSpec.cell_bytes = 3 -- the grid tensors (grid, pool_grid) ARE the reference's triples, u8[B,H,W,3]
 * (type, color, state | a box's content << 2), the tensor BASELINE.json's north star names.  The step / gen_obs kernels pack them
 * into their 16-bit LDS tile as the bytes arrive and write changed cells back as three bytes, so a caller that holds its state in
 * the reference's form pays the conversion inside the step's own launch (C4, 65536 envs: 23.6 us against 18.4 on packed cells)
 * instead of a pack and an unpack launch around it (55..62 us).  Served: mgx_gen_obs, mgx_step, mgx_step_autoreset, mgx_step_ex (steps = 1, no one_hot, no generate),
 * mgx_step_chains / mgx_sub_shards, mgx_reset_done, mgx_full_obs, mgx_launch_info; MgxStepArgs.grid_bad receives what
 * mgx_pack_grid_env would have counted.  Everything else: MGX_ERR_UNSUPPORTED.  Same results bit for bit. */

#define MGX_MAX_AGENTS 32
#define MGX_MAX_VIEW 15
#define MGX_AGENT_STRIDE 8

/* Constructor-level configuration of one env class: multigrid/base.py:85-103 plus the env-specific step hook. */
typedef struct MgxSpec {
    int32_t width;               /* grid width  W  (multigrid/base.py:152-155) */
    int32_t height;              /* grid height H */
    int32_t num_agents;          /* A */
    int32_t view_size;           /* v, odd, 3..MGX_MAX_VIEW (multigrid/core/agent.py:78-80) */
    int32_t max_steps;           /* multigrid/base.py:91 */
    int32_t see_through_walls;   /* multigrid/base.py:92 (agents[0]'s value is used for all: base.py:364-365) */
    int32_t allow_agent_overlap; /* multigrid/base.py:95 */
    int32_t joint_reward;        /* multigrid/base.py:96 */
    int32_t success_any;         /* success_termination_mode == 'any' (multigrid/base.py:97) */
    int32_t failure_any;         /* failure_termination_mode == 'any' (multigrid/base.py:98) */
    int32_t env_kind;            /* MGX_KIND_*: which subclass step() hook runs after the base step */
    int32_t cell_bytes;          /* ABI 9: the grid's cell format: 0 or 2 = MgxCell (16 bits), 1 = MgxCell8 (compact, see above),
                                    3 = the reference's byte triples u8[B,H,W,3] (see above) */
} MgxSpec;

/* Launch geometry chosen for (spec, batch); for diagnostics, benchmarks and DESIGN.md tables. */
typedef struct MgxLaunchInfo {
    int32_t envs_per_wavefront;
    int32_t envs_per_workgroup;
    int32_t threads_per_workgroup;
    int32_t workgroups;
    int32_t lds_bytes;
    int32_t slots_per_group;     /* view slots a wavefront gathers / stages as one block: 16, or 4 / 8 in the latency regime */
    int32_t fixed_shape;         /* ABI 7: > 0 = the plain step of this (spec, batch) runs a shape-specialised instantiation of the
                                    latency family (W, H, A and the envs per wavefront are compile-time constants: the shapes
                                    BASELINE.json names); 0 = the generic kernel.  Same results either way */
} MgxLaunchInfo;

int mgx_abi_version(void);
const char *mgx_error_string(int code);
int mgx_last_hip_error(void);

/* Replaces gen_obs_grid_encoding (multigrid/utils/obs.py:65-102) as called from MultiGridEnv.gen_obs
 * (multigrid/base.py:361-366), for B envs.  `dir` may be NULL. */
int mgx_gen_obs(const MgxSpec *spec, int64_t batch, const MgxCell *grid, const uint8_t *agents,
                uint8_t *obs, uint8_t *dir, void *stream);

/* Replaces MultiGridEnv.step (multigrid/base.py:303-346: step_count += 1, handle_actions 378-476, gen_obs
 * 348-376, terminations, truncations) and the BlockedUnlockPickupEnv.step post-hook
 * (multigrid/envs/blockedunlockpickup.py:166-175, redbluedoors.py:170-187, locked_hallway.py:203-227), for B envs, in one
 * fused kernel launch.
 * grid / agents / rng / step_count are updated in place. */
int mgx_step(const MgxSpec *spec, int64_t batch, MgxCell *grid, uint8_t *agents, uint64_t *rng,
             int32_t *step_count, const int8_t *actions, uint8_t *aux,
             uint8_t *obs, uint8_t *dir, double *reward, uint8_t *terminated, uint8_t *truncated,
             int32_t *err, void *stream);

/* `steps` consecutive mgx_step calls in ONE launch, bit-identical to calling mgx_step `steps` times: every wavefront
 * keeps its envs' grid tile, agent rows, PCG64 state and step counts in LDS between steps, so the per-step HBM
 * traffic is just the actions in and the outputs out, and there is no launch or state round trip per step.
 * For rollouts whose actions do not depend on the observations (scripted / random policies, the benchmark of
 * BASELINE.json); a policy in the loop needs mgx_step.
 *   actions i8[steps,B,A]   obs u8[steps,B,A,v,v,3]   dir u8[steps,B,A]   reward f64[steps,B,A]
 *   terminated u8[steps,B,A]   truncated u8[steps,B]        (state tensors as in mgx_step, updated once at the end) */
int mgx_rollout(const MgxSpec *spec, int64_t batch, int32_t steps, MgxCell *grid, uint8_t *agents, uint64_t *rng,
                int32_t *step_count, const int8_t *actions, uint8_t *aux,
                uint8_t *obs, uint8_t *dir, double *reward, uint8_t *terminated, uint8_t *truncated,
                int32_t *err, void *stream);

/* Grid format conversion on the device (the reference's Grid.state holds (type, color, state) triples):
 *   mgx_pack_grid    cells3 u8[n_cells, 3] -> packed u16[n_cells]; bad[0] (i32, device, may be NULL; the caller zeroes it)
 *                    += the number of cells with a value the packed format cannot hold (they are stored truncated)
 *   mgx_unpack_grid  packed u16[n_cells] -> cells3 u8[n_cells, 3]
 * n_cells = B*H*W for a whole grid tensor (both layouts are [b][y][x]). */
int mgx_pack_grid(const uint8_t *cells3, int64_t n_cells, MgxCell *packed, int32_t *bad, void *stream);
int mgx_unpack_grid(const MgxCell *packed, int64_t n_cells, uint8_t *cells3, void *stream);
/* (ABI 8) mgx_pack_grid for whole env grids cells3 u8[B,H,W,3]: bad is i32[2] (may be NULL; the caller zeroes it) --
 *   bad[0] += cells with a value the packed format cannot hold, bad[1] += cells of an env's outer ring that are not the
 *   reference's WALL = (wall, grey, 0) (multigrid/utils/obs.py:14; the PRECONDITION under "grid" above).
 * mgx_check_grid: the same preconditions for state that is already on the device in the packed format, opt-in (one cheap
 * kernel; nothing else in this library re-checks what it is handed):
 *   bad i32[4], the caller initialises it to {0, 0, 0, INT32_MAX}:  bad[0] += cells that are not a valid packed cell (reserved
 *   bits, type > 10, color > 5, state > 2, opaque bit inconsistent with (type, state): multigrid/utils/obs.py:46-63),
 *   bad[1] += outer-ring cells that are not WALL, bad[2] += agent rows outside the walls (x or y) / with direction > 3 / with
 *   terminated > 1 / with colour > 5 / with a carried cell the format cannot hold (its type > 10, colour > 5, state > 2, or a content
 *   that is not a box's -- on compact cells any content) (agents may be NULL: not checked), bad[3] = min index of an env with a
 *   violation.  Every count is of CELLS / ROWS: one that breaks several rules counts once. */
int mgx_pack_grid_env(const uint8_t *cells3, int64_t batch, int32_t height, int32_t width, MgxCell *packed, int32_t *bad,
                      void *stream);
int mgx_check_grid(const MgxSpec *spec, int64_t batch, const MgxCell *grid, const uint8_t *agents, int32_t *bad, void *stream);
/* (ABI 9) the same conversions for COMPACT cells (MgxCell8, spec->cell_bytes = 1): bad[0] also counts what only the compact
 * format cannot hold: a box's content, a state on anything but a door / an agent overlay, a door's state 3 and the types 11..15
 * (both would read back as one of the joint codes).  bad[0] counts cells: one that breaks several rules counts once. */
int mgx_pack_grid8_env(const uint8_t *cells3, int64_t batch, int32_t height, int32_t width, MgxCell8 *packed, int32_t *bad,
                       void *stream);
int mgx_unpack_grid8(const MgxCell8 *packed, int64_t n_cells, uint8_t *cells3, void *stream);

/* Geometry of the plain step's launch (mgx_step / mgx_step_autoreset; mgx_gen_obs bundles as many envs per wavefront or fewer). */
int mgx_launch_info(const MgxSpec *spec, int64_t batch, MgxLaunchInfo *out);

/* ABI 11: geometry of the launches that keep the envs' state in LDS between steps -- mgx_rollout* (persistent = 0) and
 * mgx_step_persistent (persistent = 1).
 * resident_shape > 0: one of the library's RESIDENT instantiations -- 64 view slots per wavefront, `slices` groups of `envs_per_slice`
 * envs stepped one after the other by the same wavefront.  Empty-16x16 x 4 agents from 16385 envs up (the value names the shape):
 *   7  one slice of 16 envs, 13216 B of LDS: 12 wavefronts per CU, 49152 envs resident at once -- mgx_rollout* up to that batch and
 *      beyond 65536 (in rounds), mgx_step_persistent up to 32768 envs (its residency check counts 8 wavefronts per CU)
 *   9  one slice in 9872 B and <= 128 VGPRs (the tile's rows share the grid's wall ring): 16 wavefronts per CU -- mgx_rollout* of 49153
 *      to 65536 envs: BASELINE.json configs[3] is ONE resident round of 4096 wavefronts
 *   8  two slices: 2048 wavefronts of 2 x 16 envs, 8 per CU -- mgx_step_persistent of 32769 to 65536 envs (a persistent launch must
 *      leave registers for the kernels that feed it; it owns every CU's LDS: what runs beside it must do without)
 * 0: the ordinary rollout kernels (32 view slots, one slice).  Same results either way, bit for bit. */
typedef struct MgxRolloutInfo {
    int32_t envs_per_slice;
    int32_t slices;              /* per wavefront; envs per wavefront = envs_per_slice * slices */
    int32_t wavefronts;          /* that own envs (mgx_step_persistent: the flags of MgxPersistent.done) */
    int32_t threads_per_workgroup;
    int32_t workgroups;
    int32_t lds_bytes;           /* per workgroup */
    int32_t resident_shape;
} MgxRolloutInfo;
int mgx_rollout_info(const MgxSpec *spec, int64_t batch, int32_t persistent, MgxRolloutInfo *out);

/* Replaces OneHotObsWrapper.one_hot (multigrid/wrappers.py:158-190; the wrapper RLlib registration applies to every
 * env, multigrid/rllib/__init__.py:110-111) for a flat array of cells:
 *   cells u8[n_cells, 3]  ->  out u8[n_cells, D],  D = dim_sizes[0] + dim_sizes[1] + dim_sizes[2]  (<= 32),
 *   out[c, off_d + cells[c, d]] = 1, off = (0, dim_sizes[0], dim_sizes[0] + dim_sizes[1]); everything else 0.
 * A value cells[c, d] >= dim_sizes[d] sets NO channel of field d (the reference's loop would run into the next field, or past the
 * row); the other fields of that cell are unaffected.
 * The reference uses dim_sizes = (11, 6, 4) (wrappers.py:139-140).  `out` must be 16-byte aligned (MGX_ERR_INVALID_ARGUMENT
 * otherwise); `cells` may have any alignment.  D > 32: MGX_ERR_UNSUPPORTED. */
int mgx_one_hot(const uint8_t *cells, int64_t n_cells, const int32_t *dim_sizes, uint8_t *out, void *stream);

/* Replaces FullyObsWrapper.observation (multigrid/wrappers.py:48-58): out u8[B, W, H, 3] = Grid.state ([x][y], the
 * reference's own orientation) with every agent's (10, color, dir) written at its position in index order,
 * terminated agents included.  An agent row with x >= W or y >= H writes nothing (no such row occurs in a reachable state: the
 * image is then the one without that agent).  One env's cells and output are staged in 64 KiB of LDS: MGX_ERR_UNSUPPORTED when
 * (cell_bytes + 3) * W * H + 96 > 65536 (cell_bytes 1 / 2 / 3: squares up to 127 / 114 / 104);
 * BatchedMultiGridEnv.full_obs builds larger grids' tensor from the unpacked grid instead. */
int mgx_full_obs(const MgxSpec *spec, int64_t batch, const MgxCell *grid, const uint8_t *agents, uint8_t *out,
                 void *stream);

/* Vector-env auto-reset (build-defined: the reference has no batching; its caller tests is_done(), base.py:534-539,
 * and calls reset(), base.py:250-301).  Every env b whose episode is over -- all agents terminated or
 * step_count >= max_steps -- is re-initialised from a pool of K pre-generated layouts
 * (pool_grid u16[K,H,W] packed cells, pool_agents u8[K,A,8], pool_aux u8[K,16] or NULL):
 *   layout = (first_env + b + episode[b] * 7919) mod K;  step_count[b] = 0;  episode[b] += 1;  was_reset[b] = 1.
 * The env's PCG64 stream is left running, as an unseeded reset() does for Empty envs.  `was_reset` may be NULL.
 * Checked by the validator mgx_reset_select shares: `step_count` and `episode` must be 4-byte aligned (MGX_ERR_INVALID_ARGUMENT
 * otherwise, as mgx_reset_select and mgx_reset_generate answer). */
int mgx_reset_done(const MgxSpec *spec, int64_t batch, int64_t first_env, int32_t pool_size, const MgxCell *pool_grid,
                   const uint8_t *pool_agents, const uint8_t *pool_aux, MgxCell *grid, uint8_t *agents,
                   int32_t *step_count, uint8_t *aux, int32_t *episode, uint8_t *was_reset, void *stream);

/* The two calls below fuse mgx_reset_done into the step: an env whose episode ended with the PREVIOUS step (all agents
 * terminated or step_count >= max_steps, base.py:534-539) is first re-initialised from the layout pool exactly as
 * mgx_reset_done defines, then the step is applied to the fresh state -- bit-identical to mgx_reset_done followed by
 * mgx_step, without the second launch.  `was_reset` (u8[B], or u8[steps,B] for the rollout; may be NULL) reports which envs
 * restarted before each step. */
typedef struct MgxAutoReset {
    int64_t first_env;            /* global index of env 0 of this shard */
    int32_t pool_size;            /* K >= 1 */
    const MgxCell *pool_grid;     /* u16[K,H,W] packed cells */
    const uint8_t *pool_agents;   /* u8[K,A,8] */
    const uint8_t *pool_aux;      /* u8[K,16]; NULL for MGX_KIND_EMPTY */
    int32_t *episode;             /* i32[B], in/out */
    uint8_t *was_reset;           /* out, may be NULL */
} MgxAutoReset;

int mgx_step_autoreset(const MgxSpec *spec, int64_t batch, const MgxAutoReset *ar, MgxCell *grid, uint8_t *agents,
                       uint64_t *rng, int32_t *step_count, const int8_t *actions, uint8_t *aux,
                       uint8_t *obs, uint8_t *dir, double *reward, uint8_t *terminated, uint8_t *truncated,
                       int32_t *err, void *stream);

int mgx_rollout_autoreset(const MgxSpec *spec, int64_t batch, int32_t steps, const MgxAutoReset *ar, MgxCell *grid,
                          uint8_t *agents, uint64_t *rng, int32_t *step_count, const int8_t *actions, uint8_t *aux,
                          uint8_t *obs, uint8_t *dir, double *reward, uint8_t *terminated, uint8_t *truncated,
                          int32_t *err, void *stream);

/* On-device episode starts.  Every env whose episode is over (the mgx_reset_done test) is
 * re-initialised by running the reference's own generation ON THE DEVICE, one lane per env, draw for draw:
 * Agent.reset + _gen_grid of multigrid/base.py:250-301 with place_obj / place_agent (base.py:604-697), RoomGrid's
 * place_in_room / reject_next_to / place_agent (multigrid/core/roomgrid.py:45-50, 238-259, 376-404) and numpy's
 * Generator(PCG64).integers (Lemire's method over PCG64's buffered 32-bit outputs).  Two generators per env, as in the
 * reference (its placement draws come from a construction-time generator, only Room.set_door_pos uses env.np_random,
 * roomgrid.py:104-106):
 *   gen_state u64[B,6]  [0..3] = the placement generator's PCG64 state (state_lo, state_hi, inc_lo, inc_hi),
 *                       [4] = its 32-bit buffer (has_uint32 << 32 | uinteger), [5] = the 32-bit buffer of env.np_random,
 *                       whose PCG64 words are the `rng` tensor of mgx_step.  In/out.
 *   blank     u16[H,W]  (packed cells) the grid before any object or agent is placed: the rooms' walls (RoomGrid, roomgrid.py:203-218),
 *                       or border walls + goal at (W-2, H-2) (EmptyEnv, multigrid/envs/empty.py:156-162).  It is what gets
 *                       copied into a restarted env's grid; the placement tests use the same layout in closed form, so it
 *                       must be exactly that (multigrid_amd.layouts.roomgrid_blank / empty_blank produce it)
 * Kinds:  MGX_GEN_EMPTY_FIXED          EmptyEnv with agent_start_pos / agent_start_dir (empty.py:164-167): no draws
 *         MGX_GEN_EMPTY_RANDOM         EmptyEnv with agent_start_pos=None: place_agent over the whole grid (empty.py:168-169)
 *         MGX_GEN_BLOCKEDUNLOCKPICKUP  multigrid/envs/blockedunlockpickup.py:142-164 (room_size; also writes aux[0..2])
 *         MGX_GEN_LOCKEDHALLWAY        multigrid/envs/locked_hallway.py:152-201 (room_size, max_hallway_keys, max_keys_per_room; the grid
 *                                      is 3 columns of rooms x num_rooms / 2 rows, num_rooms <= 16; numpy's Generator.shuffle for
 *                                      _rand_perm; writes the whole aux; `blank` = multigrid_amd.layouts.lockedhallway_blank)
 *         MGX_GEN_PLAYGROUND           multigrid/envs/playground.py:122-137 (room_size; rooms x rooms from the grid size, at most 16
 *                                      rooms; connect_all's doors are placed with env.np_random, roomgrid.py:104-124; `blank` =
 *                                      multigrid_amd.layouts.roomgrid_blank; spec->env_kind = MGX_KIND_EMPTY: no hook)
 *         MGX_GEN_REDBLUEDOORS         multigrid/envs/redbluedoors.py:142-168 (grid 2*size x size: agents placed in the middle
 *                                      room, then the red and the blue door rows drawn; writes aux[0..4]; `blank` = the outer
 *                                      walls + the room's walls, multigrid_amd.layouts.redbluedoors_blank)
 * A spec whose rooms have no cell to spare for what the generator places in them (e.g. a BlockedUnlockPickup room_size of 4 with two
 * agents, a Playground of 3x3-cell rooms for its 12 objects) is refused with MGX_ERR_UNSUPPORTED: the reference's place_obj samples
 * positions without a bound (base.py:604-669) and would never return -- here that lane would hang the device.
 * Given generators in the same state the result is byte-identical to the reference's reset() (pinned through
 * multigrid_amd/layouts.py and the reference's reset fixtures).  step_count := 0, episode += 1, was_reset (may be NULL). */
enum { MGX_GEN_EMPTY_FIXED = 0, MGX_GEN_EMPTY_RANDOM = 1, MGX_GEN_BLOCKEDUNLOCKPICKUP = 2, MGX_GEN_REDBLUEDOORS = 3,
       MGX_GEN_LOCKEDHALLWAY = 4, MGX_GEN_PLAYGROUND = 5 };

/* Staged generation (ABI 7, optional; used by mgx_step_generate / mgx_step_ex only).  A launch lasts as long as its slowest
 * wavefront, and the serial placement of one episode (~6500 cycles on one lane) in the tail of the step made the wavefront that
 * holds a finished env exactly that -- every step, at thousands of envs.  Most episodes of a random-action rollout end by
 * TRUNCATION, which is known in advance: two steps before an env's step_count reaches max_steps the step takes a snapshot of the
 * env's PCG64 state (the reference's handle_actions draws exactly A numbers per step, multigrid/base.py:396-399, so the state at
 * reset time is the snapshot advanced by A draws per remaining step), and in the NEXT launch a few extra wavefronts -- beside the
 * step's own, not behind them -- generate that env's next episode from it into the staging slot below.  When the episode then
 * ends by truncation its slot is adopted (a copy); an env that ends earlier (success / failure: its np_random is somewhere else)
 * finds no slot for its episode and is generated in the tail as before.  Same results bit for bit either way: the slot's content is
 * the same function of (gen_state, np_random at reset time) that the tail computes.  The slots are a cache, not state: any content
 * with tag -1 is valid (all of it may be dropped at any time).  All pointers NULL = no staging.
 *   grid    MgxCell[B,H,W]   agents u8[B,A,8]   aux u8[B,16] (may be NULL for MGX_KIND_EMPTY)
 *   words   u64[B,12]   [0..5] gen_state after the staged generation, [6..9] rng (env.np_random) after it,
 *                       [10..11] the snapshot: PCG64 state (lo, hi)
 *   tag     i32[B,4]    [0] the episode whose successor the slot holds (-1: none), [1] snapshot: episode, [2] snapshot: step_count,
 *                       [3] snapshot request: phase + 1 of the launch that took it, 0 = none / served
 *   phase   the caller adds 1 for every step it issues (any wrap-around is fine; a constant phase only disables the staging) */
typedef struct MgxGenStage {
    MgxCell *grid;
    uint8_t *agents;
    uint8_t *aux;
    uint64_t *words;
    int32_t *tag;
    int32_t phase;
    int32_t lead;                 /* ABI 8: the snapshot is taken `lead` steps before the truncation (0 = 2, the least the in-launch
                                     generators need; more when the generator runs beside the steps: see `external`) */
    int32_t external;             /* ABI 8: 1 = the step's launch carries NO generator wavefronts: the caller runs them as their own
                                     launches on a stream beside the steps' (mgx_stage_generate), a few steps ahead of the truncation --
                                     off the step's critical path altogether.  2 = the same, and the caller enqueues those launches on
                                     the steps' OWN stream, between two steps: no generator ever runs beside a step, so the step publishes
                                     its snapshot with plain stores (the kernel boundary orders them) instead of an agent-scope release --
                                     which writes the XCD's L2 back, ~1.5 us for the wavefront that takes a snapshot.  Do NOT pass 2 with
                                     generator launches on another stream. */
    int32_t candidates;           /* ABI 10: K > 0 = EVERY episode end an adoption (needs external == 2).  The layout stream that drives
                                     place_obj is the construction-time generator: it does not depend on WHEN the
                                     episode ends -- only the draws from env.np_random do, and the generators make at most one such draw
                                     (BlockedUnlockPickup: the door's row, roomgrid.py:104-106; the Empty / RedBlueDoors / LockedHallway
                                     generators none).  So the NEXT episode is generated while the current one runs, once per possible
                                     value of that draw: K = room_size - 2 candidates (<= 4) for BlockedUnlockPickup, 1 for the others
                                     (MGX_GEN_PLAYGROUND draws many times: not available).  mgx_stage_generate fills the candidates of every
                                     env whose slots are not its current episode's (tag[k] != episode; no snapshot, no request, `lead`
                                     only sets how often the caller launches it); a step that ENDS an episode -- truncation or success /
                                     failure alike -- makes the draw from np_random as it is then (registers) and adopts the matching
                                     candidate, requested as soon as the step's rules have run and stored in the tail; an env whose
                                     candidates are not there yet is generated in the tail.  Same results bit for bit.  The slots then are
                                       grid MgxCell[B,K,H,W]   agents u8[B,K,A,8]   aux u8[B,K,16]   words u64[B,K,6] (gen_state[0..4] after
                                       that candidate's generation)   tag i32[B,4]: [k] = the episode whose successor candidate k is
                                     (-1: none; any content with all tags -1 is valid) */
} MgxGenStage;

typedef struct MgxLayoutGen {
    int32_t kind;
    int32_t room_size;                    /* MGX_GEN_BLOCKEDUNLOCKPICKUP, MGX_GEN_LOCKEDHALLWAY, MGX_GEN_PLAYGROUND */
    int32_t start_x, start_y, start_dir;  /* MGX_GEN_EMPTY_FIXED */
    int32_t max_hallway_keys;             /* MGX_GEN_LOCKEDHALLWAY (locked_hallway.py:107) */
    int32_t max_keys_per_room;            /* MGX_GEN_LOCKEDHALLWAY (locked_hallway.py:108) */
    const MgxCell *blank;
    uint64_t *gen_state;
    MgxGenStage stage;                    /* ABI 7: staged generation of truncation resets (all NULL: off) */
} MgxLayoutGen;

int mgx_reset_generate(const MgxSpec *spec, int64_t batch, const MgxLayoutGen *gen, MgxCell *grid, uint8_t *agents,
                       uint64_t *rng, int32_t *step_count, uint8_t *aux, int32_t *episode, uint8_t *was_reset, void *stream);

/* Restart the envs the CALLER chooses (additive to ABI 11): what the reference's caller does with `env.reset(seed=s)` on any env
 * it likes, finished or not (multigrid/base.py:250-301).  mgx_reset_select is mgx_reset_done, mgx_reset_generate_select is
 * mgx_reset_generate, with the done test replaced by `select`:
 *   a chosen env      restarts exactly as the done-based call restarts a finished one (pool: layout = (first_env + b + episode[b] *
 *                     7919) mod K); step_count[b] = 0; episode[b] += 1; was_reset[b] = 1
 *   any other env     keeps every byte of its state -- a finished env that is not chosen stays finished; was_reset[b] = 0
 * rng_words != NULL re-seeds env.np_random of the chosen envs with the restart (reset(seed=...), base.py:269): the generation draws
 * from a fresh generator with these PCG64 words and no pending 32-bit half (gen_state[b][5] is not read), and `rng[b]` /
 * gen_state[b][5] come out as the generation left that generator; the pool form stores rng[b] = rng_words[b].  The placement stream
 * gen_state[b][0..4] is never re-seeded: it is the construction-time generator, which reset(seed) does not replace.
 * Limits and return codes are those of mgx_reset_done / mgx_reset_generate; rng_words 8-byte aligned; batch == 0 is a no-op.  `pool`
 * carries first_env, the layout pool, `episode` and `was_reset` (may be NULL).  The staging slots of MgxGenStage need no attention:
 * episode[b] += 1 makes every slot and pending snapshot of a chosen env stale (tag != episode). */
typedef struct MgxResetSelect {
    const uint8_t  *select;     /* u8[B]: non-zero = restart this env; NULL = every env */
    const uint64_t *rng_words;  /* u64[B,4]: PCG64 words installed as env.np_random of the selected envs
                                   (fresh generator, empty 32-bit buffer); NULL = the stream is left running */
} MgxResetSelect;

int mgx_reset_select(const MgxSpec *spec, int64_t batch, const MgxResetSelect *sel, const MgxAutoReset *pool, MgxCell *grid,
                     uint8_t *agents, uint64_t *rng, int32_t *step_count, uint8_t *aux, void *stream);
int mgx_reset_generate_select(const MgxSpec *spec, int64_t batch, const MgxResetSelect *sel, const MgxLayoutGen *gen, MgxCell *grid,
                              uint8_t *agents, uint64_t *rng, int32_t *step_count, uint8_t *aux, int32_t *episode,
                              uint8_t *was_reset, void *stream);

/* (ABI 8) The staging slots' generator as a launch of its own: serves every pending snapshot request of `gen->stage` (one lane
 * per env; envs without a request cost one load).  Enqueue it on a stream BESIDE the one the steps run on, ordered behind the step
 * that took the snapshots (an event): with gen->stage.external = 1 and a lead of a few steps the next episodes of the envs about to
 * truncate are ready when their truncating step adopts them, and no step ever waits for a generator.  A slot that is not ready in
 * time is simply not adopted (that env is generated in the tail of its step, as without staging): same results either way.
 * rng = the env.np_random words of mgx_step (read: the stream increments), episode as in mgx_step_generate. */
int mgx_stage_generate(const MgxSpec *spec, int64_t batch, const MgxLayoutGen *gen, const uint64_t *rng, const int32_t *episode,
                       void *stream);

/* mgx_step followed by mgx_reset_generate, in ONE launch: the envs whose episode ends with this step (all agents terminated
 * or step_count >= max_steps after it) are regenerated in the tail of the step's own kernel; the outputs are the step's
 * (the terminal observation); the state tensors come out holding the next episode's start.  Bit-identical to the two calls.
 * `was_reset` (may be NULL) = the envs that were regenerated. */
int mgx_step_generate(const MgxSpec *spec, int64_t batch, const MgxLayoutGen *gen, MgxCell *grid, uint8_t *agents,
                      uint64_t *rng, int32_t *step_count, const int8_t *actions, uint8_t *aux,
                      uint8_t *obs, uint8_t *dir, double *reward, uint8_t *terminated, uint8_t *truncated,
                      int32_t *err, int32_t *episode, uint8_t *was_reset, void *stream);

/* The step / gen_obs with the observation written ONE-HOT encoded: what OneHotObsWrapper.one_hot
 * (multigrid/wrappers.py:158-190, dim sizes (11, 6, 4)) makes of obs['image'], fused into the same launch -- the
 * wrapper RLlib registration applies to every env (multigrid/rllib/__init__.py:110-111).  Bit-identical to
 * mgx_gen_obs / mgx_step[_autoreset] followed by mgx_one_hot, without the 3-byte observation's round trip through HBM:
 *   obs_one_hot u8[B, A, v, v, 21]   obs_one_hot[b,a,i,j, c0] = obs_one_hot[.., 11 + c1] = obs_one_hot[.., 17 + c2] = 1
 *                                    for obs[b,a,i,j] = (c0, c1, c2); everything else 0.  16-byte aligned.
 * `ar` may be NULL (no auto-reset).  Everything else as in mgx_step / mgx_step_autoreset. */
int mgx_gen_obs_one_hot(const MgxSpec *spec, int64_t batch, const MgxCell *grid, const uint8_t *agents,
                        uint8_t *obs_one_hot, uint8_t *dir, void *stream);
int mgx_step_one_hot(const MgxSpec *spec, int64_t batch, const MgxAutoReset *ar, MgxCell *grid, uint8_t *agents,
                     uint64_t *rng, int32_t *step_count, const int8_t *actions, uint8_t *aux,
                     uint8_t *obs_one_hot, uint8_t *dir, double *reward, uint8_t *terminated, uint8_t *truncated,
                     int32_t *err, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The general form of the step (ABI 6).  Every mgx_step* / mgx_rollout* entry point above is this call with some of the
 * options set; options combine freely unless noted.  Replaces multigrid/base.py:303-346 (+ the env subclass' step hook,
 * + base.py:250-301 reset for finished envs when `auto_reset` / `generate` is given, + wrappers.py:158-190 when `one_hot`).
 *   steps        1 = one step; T > 1 = T consecutive steps in one launch (mgx_rollout: actions / hook_order / every output and
 *                was_reset carry a leading [T] axis, the state is written back once)
 *   one_hot      obs is u8[.., A, v, v, 21] (mgx_step_one_hot)
 *   auto_reset   finished envs restart from the layout pool BEFORE the step (mgx_step_autoreset), or NULL
 *   generate     the envs whose episode ends WITH the step are regenerated on the device right after it
 *                (mgx_step_generate; needs `episode`, optional `was_reset`; not together with `auto_reset`), or NULL.  With
 *                steps = T the call enqueues T launches of the step kernel over the [t] slices (generation writes the state in
 *                device memory, which the one-launch rollout keeps in LDS between its steps): same results as T calls; every
 *                slice of `obs` must then be 16-byte aligned (B * A * v * v * 3 a multiple of 16, else MGX_ERR_INVALID_ARGUMENT)
 *   hook_order   u8[B, A] or NULL: the order in which the env subclass' step hook visits the agents -- the reference's hooks
 *                iterate `actions.items()`, i.e. the insertion order of the caller's dict (multigrid/envs/redbluedoors.py:176,
 *                locked_hallway.py:210); row b lists agent indices in that order (a permutation of 0..A-1; agents absent from
 *                the dict have action -1 and are skipped wherever they are listed).  NULL = ascending index, which is what a
 *                dict built in agent order gives.  Only RedBlueDoors / LockedHallway read it (BlockedUnlockPickup's hook
 *                iterates self.agents, blockedunlockpickup.py:170).
 */
typedef struct MgxStepArgs {
    /* state, in/out */
    MgxCell *grid;
    uint8_t *agents;
    uint64_t *rng;               /* may be NULL when A == 1 */
    int32_t *step_count;
    uint8_t *aux;                /* may be NULL for MGX_KIND_EMPTY */
    /* inputs */
    const int8_t *actions;
    const uint8_t *hook_order;   /* may be NULL */
    /* outputs */
    uint8_t *obs;
    uint8_t *dir;                /* may be NULL */
    double *reward;
    uint8_t *terminated;
    uint8_t *truncated;
    int32_t *err;                /* may be NULL */
    /* options */
    int32_t steps;
    int32_t one_hot;
    const MgxAutoReset *auto_reset;
    const MgxLayoutGen *generate;
    int32_t *episode;            /* `generate`: i32[B], in/out */
    uint8_t *was_reset;          /* `generate`: u8[B] (or [T,B]), may be NULL */
    int32_t *grid_bad;           /* ABI 9, byte grids (MgxSpec.cell_bytes = 3) only, may be NULL: i32[2], the caller zeroes it --
                                    [0] += cell values the packed format cannot hold, [1] += outer-ring cells that are not WALL
                                    (the counters of mgx_pack_grid_env; nothing synchronises) */
} MgxStepArgs;

int mgx_step_ex(const MgxSpec *spec, int64_t batch, const MgxStepArgs *args, void *stream);

/* The step with a per-env LAYOUT MARKER (no ABI change: a new entry, every struct as it was).  An env that has not been written
 * since its last restart from the layout pool holds, byte for byte, one of the pool's layouts -- an Empty env for ever, any env
 * between two pickups / drops / toggles -- and the pool is small enough to stay in the caches: such an env's grid need not be
 * read from device memory at all.
 *   grid_layout  i32[B], caller-owned state, in/out, 4-byte aligned: k >= 0 = env b's `grid` equals pool_grid[k] bit for bit;
 *                -1 = nothing is known.  The marker is only a PROMISE about `grid`, which stays valid and current at all times:
 *                whoever writes an env's grid by any other way (another entry point, a copy, a torch op) stores -1 first.
 *                Arm it by comparing the grids with the pool once, or start at -1 and let the restarts arm it.
 * It is mgx_step_ex(spec, batch, args, stream) with that marker kept by the launch: a restart from the pool stores the layout's
 * index, every cell written back to `grid` stores -1.  Launches of the throughput family (more than 2048 wavefronts) with a
 * one-layout pool also READ it: a wavefront whose envs all carry the same k >= 0 fetches that layout once from the pool instead
 * of its envs' grids (grids of a power-of-two size up to 1 KiB; every other wavefront and every other launch loads the grids as
 * mgx_step_ex does).  Same results bit for bit as long as the promise holds.
 * Needs args->auto_reset (the pool), steps == 1, no generate and 16-bit cells: MGX_ERR_UNSUPPORTED otherwise.
 * grid_layout == NULL: exactly mgx_step_ex. */
int mgx_step_tracked(const MgxSpec *spec, int64_t batch, const MgxStepArgs *args, int32_t *grid_layout, void *stream);

/* Sub-shard stepping.  A launch that fills the chip in one round of wavefronts first loads (no wave has data to work on), then
 * computes, then drains, and the next step's launch cannot start before the last wave has gone; envs are independent, so the
 * same step can be issued as `parts` launches over consecutive blocks of the batch on `parts` streams, and consecutive calls
 * then form `parts` independent CHAINS of launches whose bubbles are filled by the other chains' waves (C4: 18.6 -> 16.0-16.7 us per
 * step of 65536 envs as two chains).  Blocks are cut at multiples of 64 envs; per-env seeds, auto-reset layouts and generated episodes follow
 * the global env index (auto_reset->first_env + block offset), so the results are bit-identical to mgx_step_ex on the whole batch.
 *   streams      `parts` HIP streams (hipStream_t cast to void*), one per chain
 *   fork_event   a hipEvent_t (cast to void*) the caller recorded on the stream that produced `actions`, or NULL: every chain's
 *                stream waits for it before its launch.  The call does NOT join: the outputs of block k are complete when
 *                streams[k] reaches this point (the caller makes its consumer wait on the streams it needs).
 * steps must be 1.  mgx_sub_shards() suggests `parts` for (spec, batch, options of `args`) on the current device: 1 when the
 * launch is less than two wavefronts per SIMD of the chip (splitting only shortens short launches), else 2 (round 5: two chains
 * hold their gain on every box and graph length measured -- C4 18.6 -> 16.0-16.7 us, C5 61.5 -> 47 us --, four swing between
 * 15.3 and 18.6 with the host side of the graph replay: profiles/r5_chain_policy.txt).  `args` may be NULL (plain step). */
int mgx_step_chains(const MgxSpec *spec, int64_t batch, const MgxStepArgs *args, int32_t parts, void *const *streams,
                    void *fork_event);
int mgx_sub_shards(const MgxSpec *spec, int64_t batch, const MgxStepArgs *args, int32_t *parts);

/* ---------------------------------------------------------------------------------------------------------------------
 * Shape specialisation for ANY shape, at run time (ABI 8).  The library carries shape-specialised instantiations of the step
 * kernel for the shapes BASELINE.json names (MgxLaunchInfo.fixed_shape > 0); a launch in the latency regime is a lone wavefront's
 * instruction chain, where a compile-time (W, H, A, envs per wavefront) is worth 10-14 %.  Every other shape -- the reference
 * registers 17 env ids (multigrid/envs/__init__.py:38-52) and users define their own -- gets the same treatment by compiling
 * csrc/mgx_fused.h for its geometry at run time (hipRTC; multigrid_amd/jit.py does it and caches the code object) and registering
 * the result: mgx_shape_key says what to compile for (spec, batch), mgx_shape_register loads the code object -- which must define
 * `mgx_jit_step`, `mgx_jit_step_ar` (extern "C" kernels taking the library's kernel-argument struct) and the i32 global
 * `mgx_jit_kernel_args_bytes` -- for the CURRENT device; later launches of the plain step with exactly that geometry run it
 * (mgx_step / mgx_step_autoreset / mgx_step_ex without one_hot / generate / steps > 1).  Same results bit for bit: it is the same
 * source.  Registrations live until the process ends. */
#define MGX_SHAPE_RUNTIME_COMPILED 100     /* MgxLaunchInfo.fixed_shape of a registered runtime-compiled shape */
typedef struct MgxShapeKey {
    int32_t width, height, num_agents, envs_per_wavefront, hooks, view_size, dma, stream;   /* the MGX_JIT_SHAPE initialiser, in order */
    int32_t kernel_args_bytes;   /* sizeof the kernel-argument struct of THIS library (checked against the code object's) */
    int32_t built_in;            /* out: > 0 = the library has its own instantiation for this geometry (nothing to compile) */
    int32_t registered;          /* out: a runtime-compiled one is registered for it on the current device */
} MgxShapeKey;
int mgx_shape_key(const MgxSpec *spec, int64_t batch, MgxShapeKey *key);
int mgx_shape_register(const MgxShapeKey *key, const void *code_object, size_t bytes);

/* ---------------------------------------------------------------------------------------------------------------------
 * Persistent stepping (ABI 8): closed-loop stepping without a kernel boundary per step.  Replaces the loop a caller of the
 * reference runs around multigrid/base.py:303-346 -- `obs = env.step(policy(obs))`, e.g. multigrid/rllib/__init__.py:59-63 -- for
 * batches in the latency regime (a launch of the step is a lone wavefront's instruction chain per SIMD: BASELINE.json's
 * Empty-16x16 x 4096 envs, the 8192-env share of an 8-GPU node, BlockedUnlockPickup x 16384), where the dependent-launch
 * boundary (~1.5 us) and the reload of the env state (~0.6 us) are a third of a step.
 *
 * mgx_step_persistent enqueues ONE launch of the rollout kernel (mgx_rollout: every wavefront keeps its envs' grid tile, agent
 * rows, PCG64 state and step counts in LDS) that stays resident for up to `max_steps` steps and, per step t = 1, 2, ...:
 *   (1) waits until the actions of step t are there.  They are handed over as GRANULES, one aligned 8-byte word per 4 agents of
 *       an env -- action_granules u64[B, ceil(A/4)], granule q of env b: bits [31:0] = the action bytes of agents 4q..4q+3
 *       (i8, little-endian, -1 = absent, bytes of agents >= A ignored), bits [63:32] = the tag t.  The producer writes each
 *       granule with ONE agent-scope 8-byte store (mgx_persistent_post does that from an ordinary i8[B,A] action tensor): the
 *       data is the flag, a wavefront re-reads only its own granules, no fence on either side;
 *   (2) applies the step exactly as mgx_step does (same results bit for bit, tests/test_persistent.py);
 *   (3) writes obs / dir / reward / terminated / truncated (/ was_reset) of step t THROUGH to memory -- the same buffers every
 *       step -- and then sets done[w] = t for its wavefront w.  The outputs of step t are complete once done[w] >= t for every
 *       w < waves (mgx_persistent_waves); a kernel launched after that has been observed (mgx_persistent_wait) reads them.
 * The producer may write the granules of step t+1 only after it has seen the outputs of step t complete (one action buffer,
 * one set of output buffers: the hand-shake is the double buffer).  The env state tensors of `args` (grid, agents, rng,
 * step_count, aux) are NOT current while the launch runs; they are written back when it ends: after `max_steps` steps, or after
 * the step during which ctrl[0] became non-zero (stop request), or when a wavefront has waited `timeout_ms` for its granules
 * (ctrl[1] counts those: the producer went away).  Every wait in these kernels is bounded by `timeout_ms`.
 *   ctrl u32[8], zeroed by the caller except [3] = UINT32_MAX: [0] in: stop request; [1] out: wavefronts (or waiters) that timed
 *        out; [2] out: wavefronts that have left; [3] out: min over them of the steps they completed; [4] a waiter of the
 *        hand-shake kernels timed out (shared by their wavefronts in place of LDS, which a chip-filling launch leaves none of)
 *   done u32[waves], zeroed by the caller
 * Options of `args`: auto_reset (layout pool) yes; one_hot, generate, hook_order no (MGX_ERR_UNSUPPORTED); steps is ignored.
 * Every wavefront of the launch must be resident at once: MGX_ERR_UNSUPPORTED when (spec, batch) needs more workgroups than the
 * device holds (use mgx_step for such batches: they are throughput-bound, not boundary-bound).  The launch must run on a stream
 * of its own: whatever produces the granules runs beside it. */
#define MGX_PERSIST_CTRL_WORDS 8
typedef struct MgxPersistent {
    const uint64_t *action_granules;  /* u64[B, ceil(A/4)], written by the producer */
    uint32_t *done;                   /* u32[waves] */
    uint32_t *ctrl;                   /* u32[MGX_PERSIST_CTRL_WORDS] */
    int32_t max_steps;                /* >= 1 */
    int32_t timeout_ms;               /* 1 .. 30000 */
} MgxPersistent;

int mgx_persistent_waves(const MgxSpec *spec, int64_t batch, const MgxStepArgs *args, int32_t *waves);
int mgx_step_persistent(const MgxSpec *spec, int64_t batch, const MgxStepArgs *args, const MgxPersistent *p, void *stream);
/* actions i8[B,A] (as mgx_step takes them) -> the granules of step `step` (counted from 1); stream-ordered behind whatever
 * produced `actions` on `stream`.  This call and mgx_persistent_feed find a granule's env by a 32-bit reciprocal multiply:
 * MGX_ERR_UNSUPPORTED from B * ceil(A/4) = 2^31 granules on, and already from 2^30 at 17..20 agents and from 1 431 655 766 at 25..28
 * (5 and 7 granules per env), where that quotient stops being exact.
 * Alignment (MGX_ERR_INVALID_ARGUMENT otherwise): action_granules 8 bytes; `actions` 4 bytes when A is a multiple of 4 (both calls
 * read an env's actions as dwords then), and for mgx_persistent_feed 2 bytes when A = 2 (it reads them as 16-bit words). */
int mgx_persistent_post(const MgxSpec *spec, int64_t batch, const int8_t *actions, uint32_t step, uint64_t *action_granules,
                        void *stream);
/* Returns (in stream order) once done[w] >= step for every w < waves, or after timeout_ms (then ctrl[1] += 1). */
int mgx_persistent_wait(const uint32_t *done, int32_t waves, uint32_t step, uint32_t *ctrl, int32_t timeout_ms, void *stream);
/* A stand-in policy for benchmarks and tests: a few resident workgroups (256 threads per 2048 granules) that play a recorded
 * action sequence actions i8[T,B,A]
 * through the closed-loop hand-shake -- for t = 1..T: wait for step t-1's outputs to be complete, post the granules of step t --
 * i.e. the shortest producer there can be.  trace (u64[2T + 1], may be NULL): s_memrealtime ticks (100 MHz): [2(t-1)] = step t's
 * predecessor seen complete, [2(t-1) + 1] = step t's granules posted, [2T] = step T seen complete.  A post's word is stored together
 * with the word that follows it: when a wait inside the sequence times out, the kernel ends and the words from the last post's on stay as the
 * caller left them (after steps 1 .. s were posted and step s never completed: [0 .. 2s-2] written, [2s-1 ..] not). */
int mgx_persistent_feed(const MgxSpec *spec, int64_t batch, const int8_t *actions, int32_t steps, const MgxPersistent *p,
                        int32_t waves, uint64_t *trace, void *stream);

/* RGB FRAMES (additive to ABI 11): MultiGridEnv.get_full_render (multigrid/base.py:707-760), the frame the reference's get_frame()
 * and render_mode="rgb_array" return.  A frame is a grid of tiles and a tile depends only on a key -- the cell's appearance (50:
 * empty, lava, 18 doors, 6 colours each of wall / goal, floor, key, ball, box; a box draws the same whatever it holds), the agent
 * drawn over it (none, or 6 colours x 4 directions) and whether it is highlighted -- so the 2 500 tiles are rendered once per tile
 * size into an ATLAS, bit for bit as Grid.render_tile draws them with its cache off (multigrid/core/grid.py:198-254; csrc/mgx_render.h),
 * and the frames are assembled from atlas rows.
 *   mgx_render_atlas  atlas u8[2500, tile_size, tile_size, 3]; tile_size 1..64.
 *   mgx_render        frames u8[n, H*tile_size, W*tile_size, 3] (the reference's frame layout) of the n envs grid / agents, in any
 *                     cell format of spec->cell_bytes.  The agent drawn on a cell is the highest-index NON-terminated agent there
 *                     (grid.py:281-283); a cell with terminated agents only shows none.  obs (may be NULL = no highlight) is the
 *                     mgx_gen_obs observation of the same state, u8[n, A, v, v, 3]: a cell is highlighted when it is visible
 *                     (type != unseen) in the view of any agent, terminated or not (base.py:712-747).
 * tile_size outside 1..64, or a NULL pointer with n > 0: MGX_ERR_INVALID_ARGUMENT.  Neither function synchronises. */
int mgx_render_atlas(int32_t tile_size, uint8_t *atlas, void *stream);
int mgx_render(const MgxSpec *spec, int64_t n, const MgxCell *grid, const uint8_t *agents, const uint8_t *obs, const uint8_t *atlas,
               int32_t tile_size, uint8_t *frames, void *stream);

/* VIEW FRAMES (additive to ABI 11): every agent's own view as pixels -- the partial RGB observation MiniGrid users know as
 * RGBImgPartialObsWrapper / get_frame(agent_pov=True).  Build-defined: the reference refuses it for several agents
 * (get_pov_render, multigrid/base.py), but the rule below is what its own Grid.render draws when it is handed the view as a
 * v x v Grid, the agents in it as Agents and the seen cells as the highlight mask (tests/golden/render/view_frames.npz).
 *
 * A view frame is u8[v*ts, v*ts, 3].  Pixel (py, px) belongs to view cell (i, j) = (px / ts, py / ts) of image[i, j] -- the placement
 * Grid.render uses (grid.py:291-306).  The viewer sits at (v / 2, v - 1) and faces up.  A cell's tile is the atlas tile
 * render_key(appearance, overlay, highlight) (csrc/mgx_render.h: render_view_key):
 *   appearance   of the cell's (type, color, state) exactly as the full frame computes it: unseen, empty, agent and every
 *                out-of-range byte draw no object; a box draws the same whatever it holds.
 *   another agent   a cell of type agent (10) with colour c <= 5 and state d draws overlay = 1 + 4*c + ((d - D + 3) & 3): d is the
 *                other agent's world direction, D the viewer's.  It is drawn over the empty tile (the observation does not say
 *                what lies beneath).  A colour above 5 draws no overlay.
 *   the viewer's own cell   draws the appearance of what the cell holds -- the carried object (utils/obs.py:204-207) -- under
 *                overlay = 1 + 4*own_colour + 3 (no overlay for an own colour above 5, as in the full frame).  The viewer is
 *                always drawn: the frame is a pure function of (image, direction, colour), so a terminated viewer looks like a
 *                live one.
 *   highlight    = (type != unseen) with MGX_VIEWS_HIGHLIGHT, MiniGrid's POV convention; 0 without.  Unseen cells draw the plain
 *                empty tile.
 * Any byte values are legal input: the direction counts as dir & 3, and the key is always in [0, 2500).
 *
 *   mgx_render_atlas_planar  atlas u8[2500, 3, tile_size, tile_size]: mgx_render_atlas' pixels, one plane per channel.
 *   mgx_render_views   obs u8[n_views, v, v, 3] (v = spec->view_size, the only member read), dir u8[n_views], color
 *                      u8[color_period]: view k has the own colour color[k % color_period] (the views of a trace [T, B, A, ...] need
 *                      only the B*A colours).  frames u8[n_views, P, P, 3], P = v * tile_size, from the atlas of mgx_render_atlas;
 *                      with MGX_VIEWS_PLANAR u8[n_views, 3, P, P] from the atlas of mgx_render_atlas_planar.  All offsets are 64-bit.
 *                      With tile_size % 4 == 0 and `frames` 16-byte aligned the frames are written by 16-byte stores (non-temporal
 *                      unless MGX_RENDER_STORES=plain, as mgx_render), otherwise by byte stores: same bytes.
 * Return codes: NULL spec, n_views < 0, tile_size outside 1..64, color_period < 1, an unknown flag, view_size even or outside
 * 3..MGX_MAX_VIEW: MGX_ERR_INVALID_ARGUMENT; then n_views == 0: MGX_OK, nothing is launched; then a NULL pointer:
 * MGX_ERR_INVALID_ARGUMENT; more than INT_MAX workgroups: MGX_ERR_UNSUPPORTED.  Neither function synchronises. */
enum { MGX_VIEWS_HIGHLIGHT = 1, MGX_VIEWS_PLANAR = 2 };
int mgx_render_atlas_planar(int32_t tile_size, uint8_t *atlas, void *stream);
int mgx_render_views(const MgxSpec *spec, int64_t n_views, const uint8_t *obs, const uint8_t *dir, const uint8_t *color,
                     int64_t color_period, const uint8_t *atlas, int32_t tile_size, uint32_t flags, uint8_t *frames, void *stream);

/* EPISODE ACCOUNTING (additive to ABI 11): the return, the length and the outcome of every episode, kept on the device beside the
 * envs -- what a consumer of the reference's step() return values adds up from `rewards`, `terminations` and `truncations`
 * (multigrid/base.py:338-340) and logs when an episode ends.  Build-defined like the auto-reset it follows: the reference has no
 * batching and leaves the bookkeeping to its caller.
 *
 * State, per env b, all zero at creation (MgxEpisodeStats; every pointer required):
 *   cur_return f64[B,A], cur_length i32[B]    the running episode
 *   over u8[B]                                the episode has been closed and the env has not been restarted since
 *   last_return f64[B,A], last_length i32[B]  the episode closed last
 *   sum_return f64[B,A], sum_length i64[B]    over all closed episodes
 *   counts i32[B,4]                           closed, terminated, rewarded, aborted
 *
 * mgx_episode_stats applies the outputs of `steps` consecutive steps -- reward f64[steps,B,A], terminated u8[steps,B,A], truncated
 * u8[steps,B], was_reset u8[steps,B] (required unless restart == MGX_RESTART_NONE, then ignored) -- to it, for every env and step in
 * step order:
 *   1. restart == MGX_RESTART_BEFORE and was_reset[b]: the env was restarted before this step (mgx_step_autoreset: "restarted
 *      before each step") -- the RESTART CLAUSE below.
 *   2. not over[b]:  cur_return[b,a] += reward[b,a] (one f64 add per agent and step);  cur_length[b] += 1;
 *      ended = truncated[b] != 0 || every terminated[b,a] != 0.  If ended the episode is CLOSED: last_* = cur_*;  sum_return[b,a] +=
 *      cur_return[b,a] (one f64 add per agent and close);  sum_length += cur_length;  closed++;  terminated++ if every agent was
 *      terminated;  rewarded++ if any cur_return[b,a] > 0;  cur_* = 0;  over[b] = 1.
 *   3. over[b] (as step 1 left it): a step past the end -- nothing is accumulated.
 *   4. restart == MGX_RESTART_AFTER and was_reset[b]: the env was regenerated after this step (mgx_step_generate) -- the restart
 *      clause.
 *   RESTART CLAUSE: if not over[b] and cur_length[b] > 0 the running episode is discarded (aborted++, cur_* = 0); over[b] = 0.
 * mgx_episode_restart applies the restart clause alone to the envs of `select` (u8[B], non-zero = chosen; NULL = every env): what
 * follows mgx_reset_done / mgx_reset_generate (select = their was_reset) and mgx_reset_select / mgx_reset_generate_select.
 *
 * `ended` is read from the step's OUTPUTS, the restart from the engine's own was_reset.  For every env kind but one the two agree
 * with is_done() (multigrid/base.py:534-539); LockedHallwayEnv.step reports every agent terminated once all doors are unlocked
 * without touching the agents' state (multigrid/envs/locked_hallway.py:222-225), so the engine lets such an env run on to its
 * truncation: the episode closes where the outputs say so, the steps up to the engine's restart are steps past the end, and the
 * restart opens the next episode.  Under auto-reset alone `aborted` therefore stays 0 for every env kind.
 *
 * MgxEpisodeTrace (may be NULL, and so may each of its pointers): closed u8[steps,B], episode_return f64[steps,B,A],
 * episode_length i32[steps,B], written for EVERY (step, env): the closed episode's values at a closing step, zeros elsewhere.
 *
 * Every env's arithmetic is its own, in step order, without atomics: bit for bit what a sequential model computes.
 * Return codes: a bad spec (NULL, num_agents outside 1..MGX_MAX_AGENTS), batch < 0, steps < 0, an unknown `restart`:
 * MGX_ERR_INVALID_ARGUMENT; then batch == 0 or steps == 0: MGX_OK, nothing is launched; then a missing required pointer or a
 * misaligned one (8 bytes for f64 / i64, 4 for i32): MGX_ERR_INVALID_ARGUMENT; more than INT_MAX wavefronts (one per 64 /
 * num_agents envs; the restart: one per 64 envs): MGX_ERR_UNSUPPORTED.  The grid's cell format plays no part. */
typedef struct MgxEpisodeStats {
    double *cur_return;
    int32_t *cur_length;
    uint8_t *over;
    double *last_return;
    int32_t *last_length;
    double *sum_return;
    int64_t *sum_length;
    int32_t *counts;
} MgxEpisodeStats;

typedef struct MgxEpisodeTrace {
    uint8_t *closed;
    double *episode_return;
    int32_t *episode_length;
} MgxEpisodeTrace;

enum { MGX_RESTART_NONE = 0, MGX_RESTART_BEFORE = 1, MGX_RESTART_AFTER = 2 };

int mgx_episode_stats(const MgxSpec *spec, int64_t batch, int32_t steps, const double *reward, const uint8_t *terminated,
                      const uint8_t *truncated, const uint8_t *was_reset, int32_t restart, const MgxEpisodeStats *stats,
                      const MgxEpisodeTrace *trace, void *stream);
int mgx_episode_restart(const MgxSpec *spec, int64_t batch, const uint8_t *select, const MgxEpisodeStats *stats, void *stream);

/* ENV COPY (additive to ABI 11): snapshot, restore and fork of chosen envs on the device -- what `copy.deepcopy(env)` gives a user
 * of the reference, for the envs the caller names, in ONE launch.  Build-defined: the reference has no batching.
 *
 * A STATE SET (MgxEnvRows) names the per-env rows of one holder of env state -- a live batch of envs, or a snapshot -- by pointer.
 * `rows` is the number of rows it holds; a nullable member is NULL when the set has no such row:
 *   cells       H * W * cell_bytes bytes per row, in the spec's cell format (any of the three)        required
 *   agents      u8[rows,A,8]                                                                           required
 *   rng         u64[rows,4]   env.np_random's PCG64 words                                              required
 *   step_count  i32[rows]                                                                              required
 *   aux         u8[rows,16]   the env subclass' hook state                                             nullable
 *   marker      i32[rows]     the layout marker of mgx_step_tracked                                    nullable
 *   episode     i32[rows]     the restart counter of MgxAutoReset / the generator                      nullable
 *   gen_state   u64[rows,6]   MgxLayoutGen.gen_state                                                   nullable
 *   cur_return f64[rows,A], cur_length i32[rows], over u8[rows]   the RUNNING TRIO of MgxEpisodeStats: all three, or none
 *
 * mgx_env_copy: for every pair i < n, row src_idx[i] of `src` is copied to row dst_idx[i] of `dst` (a NULL index array is the
 * identity i):
 *   MEMBERS      a member is copied when BOTH sets carry it; a member only one of them carries is left alone, except:
 *   marker       dst->marker[d] = -1 when `src` has no marker, or when marker_fill != 0 (the caller knows that the layout indices of
 *                the source no longer mean anything: another pool, another env);
 *   running trio when `dst` has it and `src` has not: cur_return = 0, cur_length = 0, over = 0 -- a fresh episode, and nothing is
 *                counted (no totals, no counters are part of a state set);
 *   stage_tag    the DESTINATION's MgxGenStage.tag (i32[rows,4]; NULL: none).  For every destination row written the slots are
 *                dropped (they are a cache: always valid): stage_mode 1 (candidates): all four words = -1; stage_mode 2 (snapshot
 *                forms): [0] = -1, [3] = 0; stage_mode 0: the tags are left alone;
 *   bad indices  a pair whose source or destination index is outside [0, rows) of its set is skipped WHOLE -- no byte of it is
 *                written -- and counted: bad[0] += 1, bad[1] = min(bad[1], i) (the convention of the step's `err` words: start them
 *                at {0, INT32_MAX}; i beyond INT32_MAX counts as INT32_MAX).  `bad` may be NULL: the pairs are skipped silently;
 *   duplicates   destination indices must be distinct: what a row named twice ends up with is unspecified (some mix of its sources'
 *                members), but never out of bounds.  Source indices may repeat: that is the fork;
 *   aliasing     no row of `src` may overlap a row of `dst`.
 * Everything else a step hands back (obs, reward, ...) is no part of a state set: mgx_gen_obs after a restore.
 *
 * Return codes: a bad spec (NULL, num_agents outside 1..MGX_MAX_AGENTS, an unknown cell_bytes), n < 0, NULL `src` / `dst`,
 * rows < 0, stage_mode outside 0..2: MGX_ERR_INVALID_ARGUMENT; then n == 0: MGX_OK, nothing is launched; then a NULL required member,
 * a running trio with only some of its three pointers, or a misaligned member -- 16 bytes for rng, aux, gen_state and stage_tag
 * (they move as 16-byte vectors), 8 for agents, cur_return and the index arrays, 4 for the i32 members and `bad`, 2 for 16-bit cells --
 * MGX_ERR_INVALID_ARGUMENT; more than INT_MAX workgroups: MGX_ERR_UNSUPPORTED. */
typedef struct MgxEnvRows {
    void *cells;
    uint8_t *agents;
    uint64_t *rng;
    int32_t *step_count;
    uint8_t *aux;
    int32_t *marker;
    int32_t *episode;
    uint64_t *gen_state;
    double *cur_return;
    int32_t *cur_length;
    uint8_t *over;
    int64_t rows;
} MgxEnvRows;

int mgx_env_copy(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, const MgxEnvRows *dst,
                 const int64_t *dst_idx, int32_t *stage_tag, int32_t stage_mode, int32_t marker_fill, int32_t *bad, void *stream);

/* STATE KEYS (additive to ABI 11): a 64-bit identity of an env's state, and of an agent's observation, made on the device in ONE
 * launch that reads the state once -- a transposition key for a search over forked envs, a cell key for an archive of snapshots,
 * the thing `torch.unique` counts for count-based exploration.  Build-defined: the reference has no such notion.
 *
 * THE RULE.  A key is the XOR of splitmix64(w ^ salt) over a set of 64-bit words w = tag << 60 | idx << 32 | payload (32-bit
 * payload).  splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) *
 * 0x94D049BB133111EB; return x ^ x >> 31 -- all mod 2^64; splitmix64(0) = 0xE220A8397B1DCDAF.  `salt` is the caller's (0 is as
 * good as any); a second salt gives an independent second key to callers who want 128 bits.  Every (tag, idx) occurs once in a key,
 * so no two terms cancel, and XOR makes the key independent of the order in which the words are visited.
 *
 * A STATE KEY covers
 *   tag 1  cells       the cell at p = y * W + x as the triple (t, col, sb) that `BatchedMultiGridEnv.grid` shows for the spec's cell
 *                      format (a box's content in the state byte included: "BOX CONTENTS"), c = (t & 15) | (col & 7) << 4 | sb << 8,
 *                      16 bits; the derived opaque bit of the packed formats is NOT part of c.  Word j (idx = j) holds the cells 2j
 *                      and 2j + 1: payload = c[2j] | c[2j + 1] << 16; with H * W odd the missing last cell is 0xFFFF.  At most
 *                      32 513 words (255 x 255 cells): idx fits 16 bits;
 *   tag 2  agents      for agent a and half h in {0, 1}: idx = 2a + h, payload = the little-endian u32 of bytes 4h .. 4h + 3 of the
 *                      agent's 8-byte row;
 *   tag 3  aux         idx 0..3, the little-endian u32s of the 16 aux bytes; a state set without `aux` is keyed as 16 zero bytes;
 *   tag 4  step count  only with MGX_KEY_STEP_COUNT: idx 0, payload = (uint32_t)step_count;
 *   tag 5  rng         only with MGX_KEY_RNG: idx 0..7, the little-endian u32 halves of the four PCG64 words.
 * Engine state is never part of a key: the layout marker, the episode counter, the generator's words, the running episode.
 * It follows that
 *   * the same reference-visible state has the same key in all three cell formats (16-bit, compact, byte triples);
 *   * byte-grid values outside the packed format (the ones `grid_bad` counts) are keyed after the masks above.
 *
 * An OBSERVATION KEY covers one agent view:
 *   tag 8  image       idx = j over the ceil(3 * v * v / 4) little-endian u32s of the view's v * v * 3 image bytes, zero-padded at
 *                      the tail;
 *   tag 9  direction   idx 0, payload = dir.
 * The agent's index is no part of it: two agents that see the same thing have the same key.
 *
 * mgx_state_key: keys[i] = the key of row src_idx[i] of the state set `src` (a NULL src_idx is the identity i; indices may repeat),
 * i < n.  An index outside [0, rows) leaves keys[i] untouched and is counted as mgx_env_copy counts a bad pair: bad[0] += 1,
 * bad[1] = min(bad[1], i); `bad` may be NULL.  Of `src` only cells, agents, step_count, rng (required) and aux (nullable) are read.
 * Return codes: a bad spec (as mgx_env_copy), n < 0, NULL `src`, rows < 0, an unknown flag: MGX_ERR_INVALID_ARGUMENT; then n == 0:
 * MGX_OK, nothing is launched; then a NULL required member or NULL `keys`, or a misaligned pointer -- 16 bytes for rng and aux, 8 for
 * agents, `keys` and the index array, 4 for step_count and `bad`, 2 for 16-bit cells -- MGX_ERR_INVALID_ARGUMENT; more than INT_MAX
 * workgroups, or more than 2^17 cells per env: MGX_ERR_UNSUPPORTED.
 *
 * mgx_obs_key: keys[i] = the key of view i of obs u8[n_views,v,v,3] (contiguous, any alignment) and dir u8[n_views], v =
 * spec->view_size.  Return codes: NULL spec, n_views < 0, view_size outside 1..MGX_MAX_VIEW: MGX_ERR_INVALID_ARGUMENT; then
 * n_views == 0: MGX_OK; then a NULL pointer or `keys` not 8-byte aligned: MGX_ERR_INVALID_ARGUMENT; more than INT_MAX workgroups:
 * MGX_ERR_UNSUPPORTED. */
enum { MGX_KEY_STEP_COUNT = 1, MGX_KEY_RNG = 2 };

int mgx_state_key(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, uint32_t flags, uint64_t salt,
                  int64_t *keys, int32_t *bad, void *stream);
int mgx_obs_key(const MgxSpec *spec, int64_t n_views, const uint8_t *obs, const uint8_t *dir, uint64_t salt, int64_t *keys,
                void *stream);

/* ACTION MASKS (additive to ABI 11): which of the 7 actions of an agent can do anything in the state it is in, for chosen rows of a
 * state set, made on the device in ONE launch -- what a tree search needs before it forks one child per action, and what invalid-
 * action masking wants next to the observation.  Build-defined: the reference has no such notion.
 *
 * THE RULE.  A mask is one byte per agent: bit k stands for action k (left 0, right 1, forward 2, pickup 3, drop 4, toggle 5,
 * done 6: multigrid/core/actions.py:5-15); bit 6 and bit 7 are always 0.  For agent row r of an env, with (fx, fy) its front position
 * (position + DIR_TO_VEC[dir]) and c the front cell as `BatchedMultiGridEnv.grid` shows it:
 *   terminated  a terminated agent has mask 0;
 *   turns       bits 0 and 1 are set for every agent that is not terminated;
 *   outside     if (fx, fy) lies outside [0, W) x [0, H), bits 2..5 are clear and NO cell is read;
 *   forward     c is empty, goal, floor, lava or an open door -- and allow_agent_overlap holds, or no agent row of the env has the
 *               position (fx, fy): terminated agents count here (multigrid/base.py:425-429);
 *   pickup      the agent carries nothing and c is a key, ball or box;
 *   drop        the agent carries something, c is empty, and no agent row of the env has the position (fx, fy);
 *   toggle      one of: c is a box; c is a door whose toggle changes it -- not locked, or locked while the agent carries a key of
 *               the door's colour; in a MGX_KIND_REDBLUEDOORS env with the stale flag aux[4] set, (fx, fy) is the blue door
 *               (aux[0], aux[1]) -- that door's OBJECT is closed whatever the grid shows, which `forward` sees too; in a
 *               MGX_KIND_RULES env, some declared MGX_RULE_TOGGLES_AT rule k < aux[0] names (fx, fy), whatever its condition
 *               (deliberately conservative: such a rule can end an episode by a toggle at a cell that holds nothing toggleable).
 * This is `go && (nrow != row || writes)` of the step kernels' evaluation of one agent's action (csrc/mgx_rules.h: eval_agent) for
 * the actions 0..5, plus the RULES clause; csrc/mgx_action_mask.h states it for both compilers.  Two guarantees:
 *   SOUND   a clear bit means: the step in which this agent takes that action and every other agent takes `done` equals the step in
 *           which it takes `done` too -- in state, aux, rewards and terminated flags.  It holds for the states reached by stepping
 *           from generated, pool or reference states;
 *   TIGHT   for every env kind but MGX_KIND_RULES: a set bit means that step differs from the all-`done` step in the grid or the
 *           agent rows.
 * A mask does not depend on the cell format (of a byte-grid value it sees type & 15, colour & 7, state & 3: the masks of STATE KEYS),
 * nor on what a box holds.  It never reads or writes engine state: the layout marker, the episode counter, the generator's words,
 * the running episode, np_random, the step count.
 *
 * mgx_action_mask: mask[i, a] = the mask of agent a of row src_idx[i] of the state set `src` (a NULL src_idx is the identity i;
 * indices may repeat), i < n: u8[n, A].  With MGX_MASK_EXPAND the output is u8[n, A, 7] of 0 / 1, byte k = bit k (a `bool` tensor's
 * bytes: `logits.masked_fill(~mask, -inf)`).  `mask` may have any alignment.  An index outside [0, rows) leaves its A (or 7 A)
 * output bytes untouched and is counted as mgx_state_key counts it: bad[0] += 1, bad[1] = min(bad[1], i); `bad` may be NULL.  Of
 * `src` only cells and agents (required) and aux (nullable: no stale door, no rules) are read.
 * Return codes, in mgx_state_key's order: a bad spec (as mgx_env_copy), n < 0, NULL `src`, rows < 0, an unknown flag:
 * MGX_ERR_INVALID_ARGUMENT; then n == 0: MGX_OK, nothing is launched; then NULL cells, agents or `mask`, or a misaligned pointer --
 * 16 bytes for aux, 8 for agents and the index array, 4 for `bad`, 2 for 16-bit cells -- MGX_ERR_INVALID_ARGUMENT; more than INT_MAX
 * workgroups, or more than 2^17 cells per env: MGX_ERR_UNSUPPORTED. */
enum { MGX_MASK_EXPAND = 1 };

int mgx_action_mask(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, uint32_t flags, uint8_t *mask,
                    int32_t *bad, void *stream);

/* DISTANCE FIELDS (additive to ABI 11): how many moves it takes, walls respected, from every cell of a grid -- and from every agent --
 * to the nearest of a set of source cells, for chosen rows of a state set, made on the device in ONE launch: the heuristic of a
 * best-first search over forked envs, the potential of a shaped reward, "is this layout solvable at all".  Build-defined: the
 * reference has no such notion.
 *
 * CELL VALUES.  A cell is seen as `BatchedMultiGridEnv.grid` shows it: type & 15, colour & 7, state & 3 (the masks of STATE KEYS).  A
 * box's content is never looked at.  The field does not depend on the cell format.
 *
 * PASSABLE.  A cell is passable when its type is empty (1), floor (3), goal (8) or lava (9), or a door (4) with state open (0):
 * exactly the cells `forward` of ACTION MASKS enters when nobody stands there.  Type 0 and every other type are impassable.  Agents
 * never block: the field is static geometry.  A stale RedBlueDoors door counts as the grid shows it (aux is not read).  The flags
 * widen or narrow the set:
 *   MGX_DIST_THROUGH_CLOSED   doors with state closed (1) are passable
 *   MGX_DIST_THROUGH_LOCKED   doors with state locked (2) are passable      (a door with state 3 never is)
 *   MGX_DIST_THROUGH_OBJECTS  key (5), ball (6) and box (7) cells are passable
 *   MGX_DIST_AVOID_LAVA       lava is impassable
 *
 * SOURCES.  The members of the query MgxDistance; a cell is a source when any of them names it:
 *   type_mask, colour_mask   bit t of type_mask: every cell of type t (0..15) whose colour c has bit c of colour_mask set; 0xFF = any
 *                            colour.  colour_mask plays no part in the other selectors;
 *   agent_mask               bit a: the position of agent row a < A, terminated or not, if it lies inside the grid (bits >= A: ignored);
 *   points, num_points       i16[n, num_points, 2] of (x, y), per OUTPUT row i (not per source row).  A point outside the grid is
 *                            ignored.  NULL with num_points 0: none;
 *   flags                    the MGX_DIST_* above.
 * A source need not be passable: the distance to a key is the distance to the key's own cell.
 *
 * THE FIELD.  Level 0 = the sources.  Level k + 1 = the 4-neighbours (x +- 1, y) and (x, y +- 1) of the cells of level k that are
 * passable and in no earlier level.  d(p) = the level of p, and -1 for a cell in no level: walls, unreachable cells, every cell of an
 * env without sources.  Distances count MOVES, not actions: turns are free (an agent that has to turn first needs more actions than
 * d says).  Every distance is < H * W <= 4096.
 *
 * mgx_distance: for row src_idx[i] of the state set `src` (a NULL src_idx is the identity i; indices may repeat), i < n,
 *   field       i16[n, H, W]   d of every cell                                                              nullable
 *   agent_dist  i16[n, A]      d at agent row a's position, -1 if that lies outside the grid; a terminated agent is answered like
 *                              any other                                                                    nullable
 * At least one of the two must be given.  An index outside [0, rows) leaves its rows of both outputs untouched and is counted as
 * mgx_action_mask counts it: bad[0] += 1, bad[1] = min(bad[1], i); `bad` may be NULL.  Of `src` only cells and agents are read.  The
 * entry point never reads or writes engine state, aux, np_random or the step count.
 * Return codes, in mgx_action_mask's order: a bad spec (as mgx_env_copy), n < 0, NULL `src`, rows < 0, NULL `q`, an unknown flag,
 * num_points < 0: MGX_ERR_INVALID_ARGUMENT; then n == 0: MGX_OK, nothing is launched; then NULL cells or agents, both outputs NULL,
 * NULL points with num_points > 0, or a misaligned pointer -- 2 bytes for field, agent_dist, points and 16-bit cells, 8 for agents
 * and the index array, 4 for `bad` -- MGX_ERR_INVALID_ARGUMENT; then H > 64 or W > 64, or more than INT_MAX workgroups:
 * MGX_ERR_UNSUPPORTED.  The side limit is the kernel's: one lane holds one grid row as a 64-bit mask, one wavefront's 64 lanes the
 * rows of an env.  Every BASELINE configuration (up to 64 x 64) is inside it. */
enum { MGX_DIST_THROUGH_CLOSED = 1, MGX_DIST_THROUGH_LOCKED = 2, MGX_DIST_THROUGH_OBJECTS = 4, MGX_DIST_AVOID_LAVA = 8 };

typedef struct MgxDistance {
    uint32_t type_mask, colour_mask, agent_mask, flags;
    const int16_t *points;
    int32_t num_points;
} MgxDistance;

int mgx_distance(const MgxSpec *spec, int64_t n, const MgxEnvRows *src, const int64_t *src_idx, const MgxDistance *q, int16_t *field,
                 int16_t *agent_dist, int32_t *bad, void *stream);

/* KEY TABLES (additive to ABI 11): the set of keys already seen, kept on the device -- a transposition table for a search over forked
 * envs, the cell archive of Go-Explore, visit counts for count-based exploration.  A table maps a 64-bit key (mgx_state_key,
 * mgx_obs_key, or any number of the caller's) to a stable ENTRY ID in [0, capacity): the caller keeps what it wants per entry (best
 * score, snapshot row, parent) in arrays of its own indexed by that id.  A batch of keys is inserted in TWO launches and looked up in
 * ONE, in constant memory, without host work or synchronisation, capturable in a graph.  Build-defined: the reference has no such notion.
 *
 * STORAGE.  A table is caller-owned device memory, described by MgxKeyTable:
 *   capacity   a power of two, MGX_KEY_MIN_CAPACITY (64) <= capacity <= MGX_KEY_MAX_CAPACITY (2^30): the number of slots
 *   keys       u64[capacity]   the key a slot holds; 0 = the slot is empty                                 8-byte aligned
 *   tag        u64[capacity]   epoch << 32 | (0xFFFFFFFF - i): the last call that inserted the slot's key, and the smallest index i
 *                              of that call that held it                                                   8-byte aligned
 *   born       u32[capacity]   the epoch of the call that placed the key                                  4-byte aligned
 *   visits     u32[capacity]   how often the key has been inserted (counting calls only)                   4-byte aligned
 *   ctrl       u32[MGX_KEY_CTRL_WORDS = 8]  [0] the epoch of the insert whose first launch ran last, [1] the epoch of the last
 *                              finished insert, [2] MGX_KEY_CTRL_ENTRIES: occupied slots, [3] MGX_KEY_CTRL_DROPPED: dropped indices
 *                              since the caller last zeroed the word, [4..7] zero, reserved               4-byte aligned
 * 24 * capacity + 32 bytes in all.  ALL-ZERO STORAGE IS THE EMPTY TABLE: a table is made, and cleared, by a zero fill (hipMemsetAsync
 * is capturable); epochs start at 1 again.  An epoch is a call's number, 32 bits: after 2^32 - 1 inserts without a clear the epochs
 * wrap and is_new / first are no longer right -- documented, not handled.  The caller may zero ctrl[3] at any time between calls.
 * One table takes one call at a time: two calls on one table must be ordered by their streams.
 *
 * KEY 0 marks an empty slot, so the key 0 is stored and answered as the key 1: one more 2^-64 alias, like any collision of the keys.
 *
 * PLACEMENT.  Open addressing, linear probing.  With k the canonical key (0 -> 1), home(k) = splitmix64(k) & (capacity - 1)
 * (splitmix64 of STATE KEYS: callers may pass keys that are not hash outputs).  A key is looked for, and placed, only in its WINDOW:
 * the min(MGX_KEY_MAX_PROBE = 1024, capacity) slots home, home + 1, ... taken mod capacity (the window wraps at the table's end), in
 * that order, at the first slot that holds the key or is empty.  Entries are never removed.  THE INVARIANT everything rests on: a
 * slot goes from empty to one key exactly once and never changes again -- so every slot before a key's slot in its window is
 * occupied by another key, and a lookup may stop at the first empty slot.
 *
 * mgx_key_insert(table, n, keys i64[n], flags, entry i64[n], is_new u8[n], first i64[n], visits i32[n], stream); `entry` is required,
 * is_new, first and visits are nullable.  THE RULE: apart from the VALUES of `entry`, the outputs are those of inserting keys[0..n)
 * one after another in index order.
 *   entry[i]    the id of the key's entry = its slot, in [0, capacity): equal for equal keys, different for different keys, the same
 *               in every later call until the table is cleared; -1 if the key could not be placed (FULL).  Which number an entry gets
 *               depends on the order in which the device's threads arrive and is NOT reproducible from run to run.  All below is.
 *   is_new[i]   1 iff the key was not in the table before this call and no j < i of this call holds the same key: exactly one index
 *               per new key, the smallest; else 0
 *   first[i]    the smallest j of this call with keys[j] == keys[i] (canonical keys)
 *   visits[i]   how many times the key has been inserted in the table's life by counting calls, this call included: the count AFTER
 *               the call, the same for every index of a key
 * With the flag MGX_KEY_NO_COUNT the call counts nothing (pure set semantics); visits[i] is then the count as it stood.
 * FULL: an index whose key's window holds neither the key nor an empty slot is DROPPED: entry = -1, is_new = 0, first = -1, visits = 0,
 * and ctrl[MGX_KEY_CTRL_DROPPED] goes up by one per dropped index.  All indices of a call with one key share its fate (by the
 * invariant: whoever placed the key left it where every other walk of that window meets it).  WHICH keys are dropped when more new
 * keys arrive than their windows hold is arrival order, hence unspecified; a non-zero counter has told the caller.
 * ctrl[MGX_KEY_CTRL_ENTRIES] counts the placed keys.
 *
 * mgx_key_lookup(table, n, keys i64[n], entry i64[n], visits i32[n] nullable, stream): read-only.  entry[i] = the key's entry id, -1
 * for a key the table does not hold; visits[i] its count, 0 for an absent key.
 *
 * Return codes, in mgx_state_key's order: a NULL table, a capacity that is not a power of two in range, n < 0, an unknown flag:
 * MGX_ERR_INVALID_ARGUMENT; then n == 0: MGX_OK, nothing is launched; then a NULL array of the table, NULL `keys` or `entry`, or a
 * misaligned pointer -- 8 bytes for keys, entry, first and the table's 64-bit arrays, 4 for visits and the table's 32-bit arrays --
 * MGX_ERR_INVALID_ARGUMENT; then n >= 2^31 (an index must fit the tag's low word with room to spare), or more than INT_MAX
 * workgroups: MGX_ERR_UNSUPPORTED.  csrc/mgx_key_table.h states the rule for both compilers. */
enum { MGX_KEY_NO_COUNT = 1 };
enum { MGX_KEY_MAX_PROBE = 1024, MGX_KEY_MIN_CAPACITY = 64, MGX_KEY_MAX_CAPACITY = 1 << 30, MGX_KEY_CTRL_WORDS = 8,
       MGX_KEY_CTRL_ENTRIES = 2, MGX_KEY_CTRL_DROPPED = 3 };

typedef struct MgxKeyTable {
    int64_t capacity;
    uint64_t *keys;
    uint64_t *tag;
    uint32_t *born;
    uint32_t *visits;
    uint32_t *ctrl;
} MgxKeyTable;

int mgx_key_insert(const MgxKeyTable *table, int64_t n, const int64_t *keys, uint32_t flags, int64_t *entry, uint8_t *is_new,
                   int64_t *first, int32_t *visits, void *stream);
int mgx_key_lookup(const MgxKeyTable *table, int64_t n, const int64_t *keys, int64_t *entry, int32_t *visits, void *stream);

/* SELECTION (additive to ABI 11): the k best of n, as a list of fixed length, with the count kept on the device -- the beam cut of a
 * search level, and with no scores a fixed-shape `nonzero`.  In O(n): a radix select for the threshold, then an order-preserving
 * compaction.  No host work, no synchronisation, capturable in a graph.  Build-defined: the reference has no such notion.
 *
 * mgx_select(n, score i32[n] nullable, keep u8[n] nullable, values i64[n] nullable, k, fill, index i64[k], count i32[2], work,
 * work_bytes, stream).  THE RULE:
 *   candidates  C = { i < n : keep == NULL or keep[i] != 0 } -- any non-zero byte counts
 *   m           min(k, |C|)
 *   chosen      the m candidates smallest by the pair (score[i], i); scores compare as signed int32; with score == NULL the order is
 *               by i alone.  The chosen set is that of a stable argsort of the candidates' scores, cut at m.
 *   index       index[0..m) holds the chosen i in ASCENDING i (an order-preserving compaction: with score == NULL the call is a
 *               `nonzero` of fixed shape); with `values` given, values[i] is written in place of i.  index[m..k) = fill.  No byte
 *               outside index[0..k) is written.
 *   count       count[0] = m, count[1] = |C|: the caller sees a cut as count[1] > count[0].  Both words are written by every call,
 *               never accumulated.
 * The outputs are a pure function of the inputs, byte-identical from run to run.
 *
 * WORK belongs to the caller: at least mgx_select_work_bytes(n) bytes (monotone in n), 16-byte aligned.  Its contents on entry are
 * arbitrary; the call initialises what it needs with launches of its own on `stream`, so a captured call replays correctly on new data
 * in the same arrays.  One work buffer takes one call at a time.
 *
 * LAUNCHES: six with scores, two without, one for n == 0 -- a function of the arguments, never of the data.
 *
 * Return codes, in this order: n < 0, k < 1, score and keep both NULL, NULL index or count: MGX_ERR_INVALID_ARGUMENT; then n == 0:
 * MGX_OK -- index is all `fill`, count is {0, 0}, one small launch writes them; then NULL or too small `work`, or a misaligned
 * pointer -- 8 bytes for values and index, 4 for score and count, 16 for work -- MGX_ERR_INVALID_ARGUMENT; then n or k above INT_MAX:
 * MGX_ERR_UNSUPPORTED.
 *
 * LEFT OUT ON PURPOSE: output in rank order (a flag can add it later); float scores; a device-side open list (push / pop-best) built
 * on this call; a "skip" sentinel for the row indices of mgx_env_copy and the row queries -- that would change a published contract,
 * so callers pad with a valid row.  csrc/mgx_select.h states the rule for both compilers. */
size_t mgx_select_work_bytes(int64_t n);
int mgx_select(int64_t n, const int32_t *score, const uint8_t *keep, const int64_t *values, int64_t k, int64_t fill, int64_t *index,
               int32_t *count, void *work, size_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */
