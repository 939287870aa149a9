/*
 * plantos_batch.h -- C-ABI of the MI355X-native batched PlantOSEnv step/reset.
 *
 * Drop-in boundary.  The reference has no native FFI: its
 * boundary is two Python protocols, and every entry point below replaces one of
 * them for a whole batch of N envs resident in HBM:
 *
 *   pe_create       PlantOSEnv.__init__              plantos_env.py:25-123
 *                   + DummyVecEnv(env_fns)           A2C_training.py:216-218
 *   pe_reset        PlantOSEnv.reset                 plantos_env.py:125-158
 *                   (map generation _generate_map    plantos_env.py:338-372)
 *   pe_step         PlantOSEnv.step                  plantos_env.py:160-183
 *                   + DummyVecEnv.step_wait auto-reset (SB3)
 *   pe_get_info     PlantOSEnv._get_info             plantos_env.py:317-336
 *   pe_get_state /  the state tuple MCTS clones      mcts_custom_trainer.py:236-241
 *   pe_set_state    (+ CurriculumWrapper visit_counts injection, A2C_training.py:88-93)
 *   pe_load_maps    reset() with a host-supplied layout (seed-exact CPython stream mode)
 *   pe_seed         VecEnv.seed / reset(seed=...)    (the reference ignores it for maps)
 *   pe_destroy      PlantOSEnv.close                 plantos_env.py:522-528
 *   pe_mcts_*       MCTS.search for every env at once mcts_custom_trainer.py:72-243
 *   pe_render       PlantOSEnvNew.render ('rgb_array') gradio-app/plantos_env_new.py:631-633
 *
 * Conventions
 *  - Every array argument is a DEVICE pointer (caller-owned, e.g. a torch tensor on
 *    the handle's device), row-major, env index outermost.  Only the handle's state
 *    is owned by the library.
 *  - Calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream).  They return PE_OK or a negative PE_ERR_* code; the message of
 *    the last failure on the calling thread is pe_last_error().
 *  - A handle is bound to one device and is not re-entrant.
 *  - No CPU fallback: if the HIP runtime or a gfx950 device is unavailable, pe_create
 *    fails with PE_ERR_DEVICE.
 */
#ifndef PLANTOS_BATCH_H
#define PLANTOS_BATCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_ABI_VERSION 4

enum pe_status {
    PE_OK = 0,
    PE_ERR_ARG = -1,      /* bad argument / config (Python: ValueError)            */
    PE_ERR_DEVICE = -2,   /* HIP runtime / device failure                          */
    PE_ERR_NOMEM = -3,    /* device allocation failed                              */
    PE_ERR_NOROOM = -4,   /* map generation had no room (plantos_env.py:360-364)  */
};

/* Per-env scalar slots of the canonical state (pe_get_state / pe_set_state), int32. */
enum pe_scalar {
    PE_S_X = 0,        /* rover_pos[0] (row)          plantos_env.py:96  */
    PE_S_Y = 1,        /* rover_pos[1] (column)                           */
    PE_S_STEP = 2,     /* step_count                  plantos_env.py:119 */
    PE_S_COLL = 3,     /* total_collisions            plantos_env.py:123 */
    PE_S_COLLIDED = 4, /* collided_with_wall          plantos_env.py:121 */
    PE_S_BONUS = 5,    /* completion_bonus_given      plantos_env.py:122 */
    PE_S_POISONED = 6, /* bit0: root env would raise TypeError (watering a hydrated
                          plant, plantos_env.py:217-220); bit1: action < -4 (IndexError);
                          bit2: last reset had no room (ValueError)                */
    PE_S_EPISODE = 7,  /* number of resets so far (device-rng stream index)        */
    PE_NSCAL = 8
};

/* pe_get_info columns, int32 (plantos_env.py:317-336). */
enum pe_info {
    PE_I_X = 0, PE_I_Y, PE_I_THIRSTY, PE_I_HYDRATED, PE_I_TOTAL_PLANTS, PE_I_STEP,
    PE_I_EXPLORED, PE_I_TOTAL_CELLS, PE_I_COLLIDED, PE_I_COLLISIONS, PE_I_POISONED,
    PE_NINFO
};

/* Cell codes of the canonical grid (obstacles set + plants dict, plantos_env.py:97-98). */
enum pe_cell { PE_EMPTY = 0, PE_OBSTACLE = 1, PE_HYDRATED = 2, PE_THIRSTY = 3 };

typedef struct pe_config {
    int32_t abi_version;        /* = PE_ABI_VERSION */
    int32_t grid_size;          /* G, plantos_env.py:25 (device: 1..128)        */
    int32_t num_plants;         /* P                                            */
    int32_t num_obstacles;      /* O -> O/3 clusters, plantos_env.py:341        */
    int32_t lidar_range;        /* R (device: 1..64)                            */
    int32_t lidar_channels;     /* C (device: the lane-per-env kernels' [64 x D] f32 LDS
                                   obs tile + 2CR bytes of ray offsets within 160 KiB:
                                   C <= 120 at R <= 7, fewer rays above)         */
    int32_t max_steps;          /* 1000, plantos_env.py:120                     */
    int32_t autoreset;          /* 1: pe_step resets done envs (DummyVecEnv)    */
    double thirsty_plant_prob;  /* 0.7, plantos_env.py:26                       */
    double r_goal, r_mistake, r_invalid, r_water_empty; /* plantos_env.py:76-79 */
    double r_step, r_exploration, r_revisit, r_complete; /* plantos_env.py:80-83 */
    uint64_t seed;              /* device-rng key (Philox4x32-10)               */
    uint32_t env_id_offset;     /* global id of env 0 (sharding across GPUs)    */
    int32_t map_generation_algo; /* PE_MAP_ORIGINAL (0, plantos_env.py:338-372) or
                                    PE_MAP_MAZE (the fork's map_generation_algo='maze',
                                    gradio-app/plantos_env_new.py:355-358, 408-604; G >= 7) */
    /* Auto-reset tuning (speed only: every setting gives the same results).  -1 = the
     * library's choice for the geometry (pe_default_config sets -1).              */
    int32_t coop_max_done;      /* a step-kernel block resets up to this many done envs
                                   wave-cooperatively, more one lane per env; 0 = always
                                   one lane per env                                 */
    int32_t prefetch_every;     /* steps between the launches that generate next-episode
                                   maps ahead of time; 0 = no prefetched resets       */
    int32_t obs_codes;          /* 1: the step kernel keeps the obs as byte codes (one byte
                                   per value, every value is one of < 256 table floats):
                                   pe_step_codes writes them (5C+27 B per env instead of
                                   4(5C+27)), pe_expand_obs_codes turns them into floats.
                                   Geometries whose step kernel is a sector kernel that
                                   can hold a byte-coded tile: C = 16 / R = 6 with G <= 20,
                                   C = 64 / R = 6, and every geometry of the runtime-(C, R)
                                   sector kernel (4 <= C <= 64, 2 <= R <= 14, no compile-
                                   time kernel), and the far sector kernel's C = 64 / R = 32
                                   with 96 < G + 2R <= 128; pe_create fails with PE_ERR_ARG
                                   elsewhere.
                                   pe_step still writes f32 obs on such a handle.
                                   0 (default): off                                     */
    int32_t reserved[3];
} pe_config;

enum pe_map_algo { PE_MAP_ORIGINAL = 0, PE_MAP_MAZE = 1 };

typedef struct pe_handle pe_handle;

/* Fill `c` with the reference defaults for the given geometry
 * (plantos_env.py:25-27, 76-83, 120). */
void pe_default_config(pe_config* c, int32_t grid_size, int32_t num_plants, int32_t num_obstacles,
                       int32_t lidar_range, int32_t lidar_channels);

/* Observation length 5*C + 2 + 25 (plantos_env.py:55-57). */
int32_t pe_obs_dim(const pe_config* c);

/* Allocate the SoA state for n_envs envs on `device`. All envs start reset (episode 0). */
int pe_create(const pe_config* c, int32_t device, int32_t n_envs, pe_handle** out);
int pe_destroy(pe_handle* h);

/* Re-key the device RNG (and optionally zero the episode counters), ordered on
 * `stream` after the work already queued there (step / prefetch kernels). */
int pe_seed(pe_handle* h, uint64_t seed, int32_t reset_episode_counters, void* stream);

/* Reset the envs whose mask byte is non-zero (all envs when mask == NULL) with the
 * device-rng map generator, then write obs[n_envs, D] for ALL envs (reset ones get
 * their fresh obs, the others their current obs). */
int pe_reset(pe_handle* h, const uint8_t* mask_or_null, float* obs, void* stream);

/* One step of every env.
 *   actions      int32[n] or int64[n] (action_bytes = 4 or 8); 0..3 move N/E/S/W, >=4 water
 *   obs          f32[n, D]   post-step obs (post-reset obs for done envs when autoreset)
 *   reward       f32[n]      reward (computed in f64 like the reference, cast once)
 *   terminated   u8[n], truncated u8[n]
 *   terminal_obs f32[n, D] or NULL: rows of done envs receive the pre-reset obs
 *   episode_return f64[n] or NULL: rows of done envs receive the episode's f64 return
 *   episode_length i32[n] or NULL: rows of done envs receive the episode length
 *   terminal_info  i32[n, PE_NINFO] or NULL: rows of done envs receive _get_info of the
 *                  final (pre-reset) state (DummyVecEnv keeps that step's info dict)
 * Only rows of done envs are written in the four terminal outputs (autoreset on).   */
int pe_step(pe_handle* h, const void* actions, int32_t action_bytes, float* obs, float* reward,
            uint8_t* terminated, uint8_t* truncated, float* terminal_obs_or_null,
            double* episode_return_or_null, int32_t* episode_length_or_null,
            int32_t* terminal_info_or_null, void* stream);

/* pe_step with the obs as byte codes (handles created with obs_codes = 1):
 * obs_codes u8[n, D] instead of f32[n, D]; every other argument as pe_step.  This is
 * the host-boundary form of a sharded job (plantos_amd/shard.py): ranks gather 5C+27 B
 * per env instead of 4(5C+27), and the root expands the codes once. */
int pe_step_codes(pe_handle* h, const void* actions, int32_t action_bytes, uint8_t* obs_codes, float* reward,
                  uint8_t* terminated, uint8_t* truncated, float* terminal_obs_or_null,
                  double* episode_return_or_null, int32_t* episode_length_or_null,
                  int32_t* terminal_info_or_null, void* stream);

/* The float of every obs byte code (table f32[256], host memory; unused codes 0.0). */
int pe_obs_code_table(const pe_handle* h, float* table);

/* Expand `blocks` packed code buffers into contiguous outputs.  Block b starts at
 * src + b * src_stride (bytes, a multiple of 16) and holds codes u8[rows, D], then at
 * the next multiple of 16 bytes reward f32[rows], terminated u8[rows], truncated
 * u8[rows] (the io layout of plantos_amd's code-mode batches); outputs: obs
 * f32[blocks * rows, D] and (each may be NULL) reward f32 / terminated u8 / truncated
 * u8 [blocks * rows], in block order.  Any handle of the same geometry gives the same
 * table (e.g. the root rank's shard expanding every rank's gathered codes). */
int pe_expand_obs_codes(const pe_handle* h, int32_t blocks, int32_t rows, const uint8_t* src, int64_t src_stride,
                        float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, void* stream);

/* info columns (pe_info) for all envs: int32[n, PE_NINFO]. */
int pe_get_info(pe_handle* h, int32_t* info, void* stream);

/* Canonical state, reference terms: cells u8[n,G,G] (pe_cell), visits i32[n,G,G],
 * explored i8[n,G,G] (0/1/2), scalars i32[n,PE_NSCAL].  Any pointer may be NULL
 * (get: skipped; set: that part is left unchanged).  set recomputes derived
 * counters (explored/total cells) from the arrays. Visits are exact int32 counts. */
int pe_get_state(pe_handle* h, uint8_t* cells, int32_t* visits, int8_t* explored, int32_t* scalars,
                 void* stream);
int pe_set_state(pe_handle* h, const uint8_t* cells, const int32_t* visits, const int8_t* explored,
                 const int32_t* scalars, void* stream);

/* Reset k envs (env_index i32[k]) to host-supplied layouts: cells u8[k,G,G] (obstacles
 * and plants only), rover i32[k,2]; then write obs[k, D] for those envs (row j = env
 * env_index[j]).  Used by the seed-exact CPython-stream reset mode. */
int pe_load_maps(pe_handle* h, int32_t k, const int32_t* env_index, const uint8_t* cells,
                 const int32_t* rover, float* obs_k, void* stream);

/* Synthetic benchmark actions: actions[e] = philox(seed, env_id_offset+e, t) % 5. */
int pe_synth_actions(pe_handle* h, uint64_t seed, uint32_t t, int32_t* actions, void* stream);

/* Accumulated error bits OR-ed over all envs since the last call (PE_S_POISONED bit
 * layout); synchronizes the stream. */
int pe_poll_errors(pe_handle* h, int32_t* bits, void* stream);

/* Batched CurriculumWrapper, applied inside pe_step and every reset path.  The
 * reference has two variants of the class, selected by terminate_on_threshold:
 *   1  A2C_training.py:37-109 (defaults 40 / 100 / +10, 3 episodes per maze):
 *      terminated is also reported when exploration_percentage >= the env's
 *      threshold (:101-103);
 *   0  trainingCode.py:24-98 (defaults 30 / 100 / +5, 50 episodes per maze, the
 *      wrapper of its DQN / RecurrentPPO trainers): reaching the threshold only
 *      marks the maze completed (:87-89); the episode runs on until the env itself
 *      terminates or truncates.
 * Both: exploration_percentage >= threshold marks the maze completed; at reset the threshold rises by the
 * increment after a completed maze (capped), a new map starts after a completed
 * maze or max_episodes_per_maze episodes, and otherwise the new episode keeps the
 * previous episode's visit counts (explored map restarted; the reset obs shows the
 * fresh visits, as the wrapper installs them after env.reset()).  The reference's
 * "same maze" intent is not realized there either (reset seeds are ignored).
 * Enabling (re)initializes every env's record (threshold = initial, counters 0),
 * ordered on `stream`. */
int pe_curriculum_enable(pe_handle* h, double initial_threshold, double max_threshold,
                         double threshold_increment, int32_t max_episodes_per_maze,
                         int32_t terminate_on_threshold, void* stream);
int pe_curriculum_disable(pe_handle* h);
/* threshold f64[n]; counters i32[n,4] = episode_count, successful_explorations,
 * episodes_on_current_maze, flags (bit0 maze_completed, bit1 visits carried). Device. */
int pe_curriculum_get(pe_handle* h, double* threshold, int32_t* counters, void* stream);

/* Seed-exact reset layouts (host side): the reference's _generate_map
 * (plantos_env.py:338-372) on CPython's global `random` stream after
 * random.seed(seed), including CPython 3.10 set iteration order, so the maps are
 * the ones the reference produces.  Maps come out in stream order; a DummyVecEnv
 * consumes them in env-index order at reset() and then per step (done envs in
 * index order).  Feed them to pe_load_maps.  pe_pystream_next fails with
 * PE_ERR_NOROOM where the reference raises ValueError (360-364). */
typedef struct pe_pystream pe_pystream;
int pe_pystream_create(const pe_config* c, int64_t seed, pe_pystream** out);
/* next k maps: cells u8[k,G,G] (pe_cell codes), rover i32[k,2]; HOST pointers */
int pe_pystream_next(pe_pystream* s, int32_t k, uint8_t* cells, int32_t* rover);
/* random.getrandbits(32) on the stream (tests pin the number of draws consumed) */
uint32_t pe_pystream_getrandbits32(pe_pystream* s);
int pe_pystream_destroy(pe_pystream* s);

/* Batched MCTS (mcts_custom_trainer.py:72-243): one MCTS.search per env of `h`,
 * every env with its own tree, its own clone of the env state (_copy_env_state
 * :221-243: position, plants, obstacles, explored map, visit counts and step count
 * copied; collision/bonus flags start cleared) and its own np.random stream
 * (numpy legacy RandomState: np.random.seed(int) = MT19937 init_genrand; random()
 * and randint(n) as numpy draws them).  UCB1 selection (:37-60), expansion of a
 * random untried action (:117-125), the 70/30 least-visited-neighbour rollout
 * policy (:141-219, +500 when a rollout ends fully explored), backpropagation and
 * best_action (:62-69) are the reference's, bit for bit.  Sim envs water with the
 * fork's semantics (hydrated plant: R_MISTAKE).  Searches read the live state of
 * `h` and never modify it; they step nothing: apply the actions with pe_step.
 * Scratch, bytes per env (one allocation per handle, every array rounded up to 256 B, plus
 * (n_simulations + 1) * 8 per handle): G*G * 4 + (n_simulations + 1) * 32 + 2512 for the
 * clone, the tree and the stream, and the arrays of the handle's own search kernel
 * (pe_mcts_kernel_name) only: (max_depth + 4) * 8 under pe_mcts_search_kernel,
 * G*G rounded up to 16, + G*G * 8 under pe_mcts_search_lds_kernel. */
typedef struct pe_mcts pe_mcts;
int pe_mcts_create(pe_handle* h, int32_t n_simulations, double c_param, int32_t max_depth, pe_mcts** out);
/* Every pe_mcts_* call needs `h` alive, except pe_mcts_destroy, which may follow pe_destroy(h). */
int pe_mcts_destroy(pe_mcts* m);
/* np.random.seed(seeds[e]) for env e (HOST array of n, or NULL: base_seed + e). */
int pe_mcts_seed(pe_mcts* m, const uint32_t* seeds, uint32_t base_seed, void* stream);
/* Stream state in numpy's own terms (get_state()[1:3]): key u32[n,624], pos i32[n].
 * HOST arrays; synchronous. */
int pe_mcts_set_rng(pe_mcts* m, const uint32_t* key, const int32_t* pos);
int pe_mcts_get_rng(pe_mcts* m, uint32_t* key, int32_t* pos);
/* One search per env (mask u8[n] or NULL = all): actions i32[n] (masked-out envs
 * untouched); optional root children in insertion order: order i32[n,5] (action,
 * -1 pad), visits i32[n,5], value f64[n,5].  Device pointers. */
int pe_mcts_search(pe_mcts* m, const uint8_t* mask, int32_t* actions, int32_t* root_order, int32_t* root_visits,
                   double* root_value, void* stream);
/* The search kernel pe_mcts_search launches for this handle, as a static string:
 * "pe_mcts_search_lds_kernel" (sim envs in LDS: G <= 64 and 64 lanes' cell bytes and
 * draw rings within 64 KiB, which holds up to G = 29) or "pe_mcts_search_kernel"
 * (sim envs in global memory, any G). */
int pe_mcts_kernel_name(pe_mcts* m, const char** name);

/* rgb_array frames (PlantOSEnvNew.render with render_mode='rgb_array',
 * gradio-app/plantos_env_new.py:631-633, 697-762: the colour path taken when no sprite
 * loads).  s = cell_size (the reference hard-codes 30, :112), H = W = G*s, a frame is
 * u8 [H][W][3] RGB; image row <-> grid row x, image column <-> grid column y.  Layers,
 * later over earlier: background; explored cells ((200,200,200, alpha 100) blended,
 * per channel ((d<<8) + (s-d)*a + s) >> 8); obstacles; plants; the C LIDAR rays (the
 * observation's march stopped by the map edge, an obstacle or any plant; end point
 * centre + (int(h*s*sin a), int(h*s*cos a)); 1-px integer Bresenham line, both end
 * points plotted, and a disc dx*dx + dy*dy <= 4 at the end; pixels off the canvas
 * dropped); the rover cell; grid lines on pixel rows / columns j*s, j < G.  The full
 * specification heads rl-env_amd/csrc/pe_render.hip.  Sprites, 'human' windows, the
 * Ursina viewer and the root env's _render_2d are out of scope.
 *
 * pe_render_tables (host only, HOST pointers, either may be NULL): ray_ends
 * i32[C][R+1][2] = (int(h*s*sin a), int(h*s*cos a)) for ray i (a = 2*pi*i/C), h = 0..R
 * -- (column, row) pixel offsets from the rover cell's centre, h*s an integer product,
 * the rest in double, truncated toward zero; palette u8[8][3] in the order
 * background (34,139,34), explored (99,163,99), obstacle (105,105,105), thirsty
 * (255,165,0), hydrated (0,255,0), ray (100,100,255), rover (0,0,255), grid line
 * (200,200,200).  Only lidar_channels / lidar_range of `c` are read. */
int pe_render_tables(const pe_config* c, int32_t cell_size, int32_t* ray_ends, uint8_t* palette);

/* k frames: frame j shows env env_index[j] (i32[k], device), or env j when env_index is
 * NULL (then k <= n_envs); it starts at out + j * frame_stride and its rows are
 * row_stride bytes apart (row_stride >= 3W; frames of one mosaic row: frame_stride = 3W).
 * Indices may repeat and come in any order; a frame whose index is outside [0, n_envs)
 * is not written (nothing out of range is accessed).  Only the 3W bytes of the k frames'
 * H rows are written.  2 <= cell_size <= 64 and G * cell_size <= 4096, else PE_ERR_ARG,
 * as for k < 0 or bad strides.  The per-cell_size device table is built at the first
 * call with that cell_size (a blocking upload into fresh memory) and kept until
 * pe_destroy.  Reads the state only; asynchronous on `stream`. */
int pe_render(pe_handle* h, int32_t k, const int32_t* env_index_or_null, int32_t cell_size, uint8_t* out,
              int64_t frame_stride, int64_t row_stride, void* stream);

/* Policy inference: a batched SB3-shaped MLP from the obs of `h`'s envs to their next
 * actions (A2C("MlpPolicy", net_arch=[256,256]) A2C_training.py:229-247; DQN("MlpPolicy",
 * net_arch=[512,512,256]) trainingCode.py:226-246; model.predict(obs, deterministic=True)
 * in the evaluation loops).  Learners stay out of scope.
 *
 * Definition (the host twin pe_policy_forward_host executes it literally; the kernel gives
 * the same bits):
 *  - A policy is 1 or 2 towers over the same obs row x[0..D), D = 5C + 27.  A tower is
 *    1..3 hidden Linear layers (widths multiples of 32 in 32..512) and a head Linear;
 *    weights in torch's nn.Linear layout (weight[out][in] row-major, bias[out]), f32.
 *    Tower 0's head has A outputs, 2 <= A <= 8 (action logits or Q-values); tower 1's
 *    head, if present, has 1 output (the value).  That is SB3 2.2.1's ActorCriticPolicy
 *    with separate pi / vf nets (Tanh) and DQN's QNetwork (one tower, ReLU); anything else
 *    is PE_ERR_ARG.
 *  - Pre-activation z_j: ONE f32 fma chain, acc = b_j; for k = 0..K-1 ascending:
 *    acc = fmaf(w[j][k], x[k], acc).  No split-K, no other association (zero padding after
 *    k = K-1 cannot change a value and is allowed).
 *  - One activation for all hidden layers, none on the heads: PE_ACT_RELU is
 *    z > 0 ? z : 0; PE_ACT_TANH is pe_tanhf, a function this project defines
 *    (rl-env_amd/csrc/pe_policy_math.hpp) from fmaf, f32 add / mul / div and bit
 *    operations only, identical on host and device (worst error against tanh: DESIGN.md
 *    section 4).
 *  - PE_POLICY_ARGMAX: the first index of the maximum of tower 0's head (torch.argmax;
 *    deterministic=True of the A2C policy, DQN's greedy action).
 *  - PE_POLICY_SAMPLE: u = (philox4x32-10(ctr = (t, env_id_offset + e, 0, 0x594C4F50),
 *    key = seed).x >> 8) * 2^-24 (pe_synth_actions' counter layout, another domain word);
 *    p_a = pe_expf(l_a - max l) (the project's exp, same header); cumulative sums in action
 *    order in f32, S the last; the action is the first a with u * S < cum_a, else A - 1.
 *    The sampler is this project's own: SB3 draws from torch's generator, which is not
 *    reproduced.
 *
 * pe_policy_tower carries a tower's shape and, for load / the host twin, its tensors:
 * weight[l] / bias[l] of Linear l (hidden layers in order, then the head). */
enum pe_activation { PE_ACT_TANH = 0, PE_ACT_RELU = 1 };
enum pe_policy_mode { PE_POLICY_ARGMAX = 0, PE_POLICY_SAMPLE = 1 };
typedef struct pe_policy_tower {
    int32_t n_hidden;          /* 1..3 */
    int32_t hidden[3];         /* widths of the hidden layers */
    int32_t n_out;             /* head outputs: A (tower 0) or 1 (tower 1) */
    int32_t reserved[3];
    const float* weight[4];    /* n_hidden + 1 tensors f32[out][in] (pe_policy_create ignores them) */
    const float* bias[4];      /* n_hidden + 1 tensors f32[out] */
} pe_policy_tower;
typedef struct pe_policy pe_policy;

/* Shapes only: allocates the packed device weights (zeroed) for `h`'s obs length and
 * chooses the kernel's env tile.  env_tile: envs per workgroup, 32 or 64, or 0 for the
 * library's choice (speed only: every tile gives the same results); PE_ERR_ARG if the
 * tile's activations do not fit the 160 KiB of LDS (512-wide layers need 32).
 * The policy must be destroyed before `h`. */
int pe_policy_create(pe_handle* h, int32_t n_towers, const pe_policy_tower* shapes, int32_t activation,
                     int32_t env_tile, pe_policy** out);
int pe_policy_destroy(pe_policy* p);
/* Repack the caller's DEVICE tensors (towers[i].weight / bias) into the policy's own
 * layout: one kernel, asynchronous on `stream`, no allocation (a learner calls it after
 * every optimizer step).  The shapes are the ones given to pe_policy_create. */
int pe_policy_load(pe_policy* p, const pe_policy_tower* towers, void* stream);
/* One forward of all n envs of the handle: obs u8[n, D] byte codes as pe_step_codes
 * writes them (obs_is_codes = 1; handles created with obs_codes; decoded through
 * pe_obs_code_table's table) or f32[n, D] as pe_step / pe_reset write them.  actions
 * i32[n]; head0 f32[n, A] and head1 f32[n] may be NULL (head1 must be NULL for a
 * one-tower policy).  seed / t are read in PE_POLICY_SAMPLE mode only.  One kernel, no host
 * sync, no allocation: graph-capturable. */
int pe_policy_forward(pe_policy* p, const void* obs, int32_t obs_is_codes, int32_t mode, uint64_t seed,
                      uint32_t t, int32_t* actions, float* head0_or_null, float* head1_or_null, void* stream);
/* pe_policy_forward in PE_POLICY_ARGMAX mode over `rows` >= 1 rows of obs instead of the
 * handle's n envs (a sampled minibatch; rows may be smaller or larger than n): obs u8[rows, D]
 * or f32[rows, D], actions i32[rows], head0 f32[rows, A] / head1 f32[rows] or NULL.  The
 * same kernel with another row count: row r has the bits pe_policy_forward_host gives for
 * that row.  Nothing past row rows - 1 is read or written.  PE_ERR_ARG for rows < 1, a
 * recurrent policy, and what pe_policy_forward refuses. */
int pe_policy_forward_rows(pe_policy* p, int32_t rows, const void* obs, int32_t obs_is_codes, int32_t* actions,
                           float* head0_or_null, float* head1_or_null, void* stream);
/* The host twin: the definition above in plain C++ on HOST arrays (no handle, no device).
 * obs f32[n, D]; towers with host tensors; outputs as pe_policy_forward (head0 / head1
 * may be NULL). */
int pe_policy_forward_host(int32_t n, int32_t D, int32_t n_towers, const pe_policy_tower* towers,
                           int32_t activation, const float* obs, int32_t mode, uint64_t seed,
                           uint32_t env_id_offset, uint32_t t, int32_t* actions, float* head0_or_null,
                           float* head1_or_null);
/* pe_tanhf (which = 0) / pe_expf (1) / pe_sigmoidf (2) of n host floats (tests and the
 * accuracy tool measure them). */
int pe_policy_math_host(int32_t which, int32_t n, const float* x, float* y);
/* Envs per workgroup of the forward kernel (introspection). */
int32_t pe_policy_env_tile(const pe_policy* p);

/* Recurrent policy inference: sb3_contrib's RecurrentActorCriticPolicy with n_lstm_layers = 1
 * and no shared LSTM (RecurrentPPO("MlpLstmPolicy", policy_kwargs=dict(lstm_hidden_size=H,
 * n_lstm_layers=1, enable_critic_lstm=True, net_arch=[128,128])), trainingCode.py:140-162;
 * model.predict(obs, state=lstm_states, episode_start=episode_start, deterministic=True),
 * trainingCode.py:413-434).  A recurrent policy is a pe_policy too: pe_policy_destroy and
 * pe_policy_env_tile serve it; pe_policy_load / pe_policy_forward on it are PE_ERR_ARG, as
 * are the *_lstm calls on a feed-forward policy.
 *
 * Definition (the host twin pe_policy_lstm_forward_host executes it literally; the kernel
 * gives the same bits):
 *  - 1 or 2 towers over the same obs row x[0..D).  Tower 0 is lstm_actor ->
 *    mlp_extractor.policy_net -> action_net; tower 1, if present, is lstm_critic ->
 *    mlp_extractor.value_net -> value_net (enable_critic_lstm=True).  Actor-only (1 tower)
 *    is what predict() evaluates.  The critic as a Linear (enable_critic_lstm=False) and
 *    shared_lstm=True are not supported.  Every tower has its own state (h, c) per env,
 *    f32[H] each; H is the same for both towers, a multiple of 32 in 32..512.  After the
 *    LSTM a tower is a tower of "Policy inference" above (1..3 hidden layers and a head,
 *    the same width rules) whose first layer reads h' (K = H) instead of the obs.
 *  - Episode start: a flag per env.  If it is set, h and c of every tower of that env read
 *    as +0.0f in this step (SB3's (1 - episode_start) * state, as a select: no -0).
 *  - Gate pre-activations, torch's layout: rows [0,H) i, [H,2H) f, [2H,3H) g, [3H,4H) o of
 *    weight_ih_l0 [4H][D], weight_hh_l0 [4H][H], bias_ih_l0, bias_hh_l0 [4H].  Each is ONE
 *    f32 chain: acc = bias_ih[j] + bias_hh[j] (one f32 add); acc = fmaf(w_ih[j][k], x[k],
 *    acc) for k ascending over D; then acc = fmaf(w_hh[j][k], h[k], acc) for k ascending
 *    over H.  No split-K (zero padding inside the chain is allowed).
 *  - Cell: pe_sigmoidf(z) = fmaf(0.5f, pe_tanhf(0.5f * z), 0.5f);
 *    c' = fmaf(sigma(z_f), c, sigma(z_i) * pe_tanhf(z_g)) (the product rounded once);
 *    h' = sigma(z_o) * pe_tanhf(c').  (h', c') replace the env's state.
 *  - The MLP, heads, argmax and sampler are those of "Policy inference", the Philox
 *    counter layout and domain word included.
 *
 * pe_policy_lstm carries one tower's LSTM: its size and, for load / the host twin, tensors. */
typedef struct pe_policy_lstm {
    int32_t hidden;            /* H */
    int32_t reserved[3];
    const float* weight_ih;    /* f32[4H][D] (pe_policy_create_lstm ignores the tensors) */
    const float* weight_hh;    /* f32[4H][H] */
    const float* bias_ih;      /* f32[4H] */
    const float* bias_hh;      /* f32[4H] */
} pe_policy_lstm;

/* Shapes only: allocates the packed device weights and the per-env state (both zeroed: a
 * fresh policy's first forward behaves as an episode start) and chooses the env tile
 * (env_tile as in pe_policy_create).  PE_ERR_ARG with a message if H is not a multiple of
 * 32 in 32..512 (larger LSTMs need a K-streamed kernel this library does not have), or if
 * a tile's images do not fit the 160 KiB of LDS (H = 512 needs env_tile 32). */
int pe_policy_create_lstm(pe_handle* h, int32_t n_towers, const pe_policy_lstm* lstms, const pe_policy_tower* shapes,
                          int32_t activation, int32_t env_tile, pe_policy** out);
/* Repack the caller's DEVICE tensors: kernels only, asynchronous on `stream`, no allocation. */
int pe_policy_load_lstm(pe_policy* p, const pe_policy_lstm* lstms, const pe_policy_tower* towers, void* stream);
/* One recurrent forward of all n envs: obs / mode / seed / t / outputs as pe_policy_forward.
 * start_a, start_b: device u8[n] or NULL; env e starts an episode if either flag is
 * non-zero (the step's terminated and truncated buffers fit as they are).  Updates the
 * policy's state in place.  One kernel, no host sync, no allocation: graph-capturable. */
int pe_policy_forward_lstm(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* start_a_or_null,
                           const uint8_t* start_b_or_null, int32_t mode, uint64_t seed, uint32_t t, int32_t* actions,
                           float* head0_or_null, float* head1_or_null, void* stream);
/* Zero the state of every env and tower (asynchronous on `stream`). */
int pe_policy_lstm_reset_state(pe_policy* p, void* stream);
/* Copy tower `tower`'s state to / from device tensors f32[n][H] (SB3's (1, n_envs, H));
 * h or c may be NULL to skip it.  Asynchronous on `stream`. */
int pe_policy_lstm_get_state(pe_policy* p, int32_t tower, float* h_or_null, float* c_or_null, void* stream);
int pe_policy_lstm_set_state(pe_policy* p, int32_t tower, const float* h_or_null, const float* c_or_null,
                             void* stream);
/* The host twin on HOST arrays: obs f32[n][D]; start u8[n] or NULL; h_state / c_state
 * f32[n_towers][n][H], updated in place; lstms / towers with host tensors; mode and outputs
 * as pe_policy_forward_host. */
int pe_policy_lstm_forward_host(int32_t n, int32_t D, int32_t n_towers, const pe_policy_lstm* lstms,
                                const pe_policy_tower* towers, int32_t activation, const float* obs,
                                const uint8_t* start_or_null, float* h_state, float* c_state, int32_t mode,
                                uint64_t seed, uint32_t env_id_offset, uint32_t t, int32_t* actions,
                                float* head0_or_null, float* head1_or_null);

/* Value-only forward: the critic tower alone, for the callers that need values and nothing
 * else (the time-limit bootstrap and last_values of a rollout; sb3_contrib's
 * predict_values(obs, lstm_states, episode_starts), which leaves the caller's state alone).
 *
 * Definition:
 *  - Env e is selected iff (want == NULL || want[e] != 0) && !(unless != NULL && unless[e] != 0);
 *    want / unless are device u8[n] (a step's truncated and terminated buffers fit as they are:
 *    the envs cut by the time limit only).
 *  - For a selected env, values[e] has exactly the bits pe_policy_forward / pe_policy_forward_lstm
 *    would write to head1[e] for the same obs -- in the recurrent case the same obs, start flags
 *    and current state.  The host twins' head1 is therefore the definition here too; there is no
 *    twin of its own.
 *  - For an env that is not selected, values[e] is not written.
 *  - Nothing else is written: the LSTM state of no env and no tower changes, tower 0 is not
 *    evaluated, no action is computed, the sampler is not touched.
 * One kernel, no host sync, no allocation: graph-capturable.  A workgroup none of whose envs is
 * selected returns at once, so a sparse selection costs about one empty launch.  PE_ERR_ARG for
 * a one-tower policy, a NULL obs or values, and the wrong kind of policy (pe_policy_value on a
 * recurrent policy, pe_policy_value_lstm on a feed-forward one); obs / obs_is_codes as
 * pe_policy_forward, start_a / start_b as pe_policy_forward_lstm. */
int pe_policy_value(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* want_or_null,
                    const uint8_t* unless_or_null, float* values, void* stream);
int pe_policy_value_lstm(pe_policy* p, const void* obs, int32_t obs_is_codes, const uint8_t* start_a_or_null,
                         const uint8_t* start_b_or_null, const uint8_t* want_or_null, const uint8_t* unless_or_null,
                         float* values, void* stream);

/* Reduced-precision policy inference: the MLP policy of "Policy inference" with bf16 operands
 * and f32 accumulation (v_mfma_f32_32x32x16_bf16).  Opt-in per policy; PE_PREC_F32 is the
 * definition of "Policy inference" unchanged.  Recurrent policies have no reduced precision.
 *
 * Definition (the host twin pe_policy_forward_host_bf16 executes it; a PE_PREC_BF16 policy
 * has the towers, shapes, activation, heads, argmax and sampler of "Policy inference", with
 * these differences):
 *  - Operand rounding: an obs value (tab[code] or the f32 obs entry), a hidden-layer weight
 *    and a hidden activation after pe_tanhf / pe_relu are each rounded to bf16 once, to
 *    nearest even.
 *  - Biases, head weights and all outputs stay f32.
 *  - Hidden pre-activation: z_j = f32(b_j + sum_k w[j][k] x[k]) over the bf16 operands,
 *    accumulated in f32 by the MFMA.  The products are exact in f32; the order and the
 *    internal rounding of the sum are the hardware's and are not defined.  The host twin
 *    computes the sum in f64 and rounds it to f32 once.
 *  - Head: the f32 fmaf chain in k order of "Policy inference" over the (bf16-valued) last
 *    hidden activations: given those activations it is defined bit for bit.
 *  - Consequence: where every partial sum of a pre-activation is exactly representable in
 *    f32, kernel and twin agree bit for bit.  Elsewhere a pre-activation may differ by f32
 *    summation error, which after the activation's bf16 rounding occasionally moves one
 *    hidden unit by one bf16 ulp.
 * pe_policy_load, pe_policy_forward, pe_policy_forward_rows and pe_policy_value serve a policy
 * of either precision with the same arguments and the same checks; within one precision every
 * env tile, pe_policy_forward_rows and pe_policy_value give the same bits. */
enum pe_precision { PE_PREC_F32 = 0, PE_PREC_BF16 = 1 };
/* pe_policy_create with a precision (pe_policy_create is PE_PREC_F32); PE_ERR_ARG for any
 * other value, and if the tile's bf16 images do not fit the 160 KiB of LDS. */
int pe_policy_create_prec(pe_handle* h, int32_t n_towers, const pe_policy_tower* shapes, int32_t activation,
                          int32_t env_tile, int32_t precision, pe_policy** out);
/* The precision a policy was created with (PE_PREC_F32 for a recurrent one); -1 for NULL. */
int32_t pe_policy_precision(const pe_policy* p);
/* The host twin of a PE_PREC_BF16 policy: arguments as pe_policy_forward_host. */
int pe_policy_forward_host_bf16(int32_t n, int32_t D, int32_t n_towers, const pe_policy_tower* towers,
                                int32_t activation, const float* obs, int32_t mode, uint64_t seed,
                                uint32_t env_id_offset, uint32_t t, int32_t* actions, float* head0_or_null,
                                float* head1_or_null);

/* Rollout collection: what SB3 2.2.1's OnPolicyAlgorithm.collect_rollouts and
 * RolloutBuffer.compute_returns_and_advantage add to the act / step loop (A2C(n_steps=5,
 * gamma=0.99, gae_lambda=1.0) A2C_training.py:229-247; the PPO family with n_steps=1024,
 * gamma=0.99, gae_lambda=0.95, trainingCode.py:140-162): per-step log-probs, the time-limit
 * bootstrap of truncated episodes, episode-start flags and the reverse-time GAE scan.
 * Learners stay out of scope.  All four functions work on caller-owned arrays; the device
 * ones run on the calling thread's current device, asynchronous on `stream`, with no
 * allocation and no sync (graph-capturable); the *_host twins execute the same definition
 * on host arrays and give the same bits.
 *
 * Definition, f32 throughout, every product and sum rounded on its own, nothing re-associated
 * (rl-env_amd/csrc/pe_rollout_math.hpp):
 *  - log-prob of action a under logits l[0..A): m = max l; z_k = l_k - m; S = the f32 sum of
 *    pe_expf(z_k) in action order (the sampler's S, in [1, 8]); z_a - pe_logf(S).  pe_logf is
 *    the project's own log (rl-env_amd/csrc/pe_policy_math.hpp; worst error DESIGN.md 4).
 *  - record, per env e after a step: done = terminated | truncated; reward_out = reward, or
 *    reward + g * terminal_value (g = (float)gamma; the product rounded, then the sum) where
 *    terminal_value is given and truncated && !terminated (SB3's TimeLimit.truncated);
 *    start_next = done; a done env adds 1 to ep_count, episode_return (f64) to ep_return_sum
 *    and episode_length to ep_length_sum -- per env, no atomics, so deterministic.
 *  - GAE, per env e: g = (float)gamma; gl = (float)(gamma * gae_lambda) (the product in f64);
 *    last = 0; for t = T-1 .. 0: nnt = 1 - (float)(start[t+1] != 0); nv = t == T-1 ?
 *    last_values[e] : values[t+1][e]; delta = (rewards[t][e] + (g * nv) * nnt) - values[t][e];
 *    last = delta + ((gl * nnt) * last); advantages[t][e] = last; returns[t][e] = last +
 *    values[t][e].  start has T + 1 rows; row T is the last step's done flags, row 0 is not
 *    read.
 *
 * pe_rollout_record: logits f32[n, A] (2 <= A <= 8), actions i32[n], reward f32[n],
 * terminated / truncated u8[n] of the step; terminal_value f32[n] or NULL (no bootstrap);
 * episode_return f64[n] / episode_length i32[n] as pe_step wrote them, or NULL.  Outputs:
 * log_prob f32[n], reward_out f32[n] (may be `reward` itself), start_next u8[n]; the
 * accumulators ep_count i32[n], ep_return_sum f64[n], ep_length_sum i32[n] may each be NULL.
 * PE_ERR_ARG for n < 1, A outside 2..8 or a NULL required pointer. */
int pe_rollout_record(int32_t n, int32_t A, const float* logits, const int32_t* actions, const float* reward,
                      const uint8_t* terminated, const uint8_t* truncated, const float* terminal_value_or_null,
                      const double* episode_return_or_null, const int32_t* episode_length_or_null, double gamma,
                      float* log_prob, float* reward_out, uint8_t* start_next, int32_t* ep_count_or_null,
                      double* ep_return_sum_or_null, int32_t* ep_length_sum_or_null, void* stream);
int pe_rollout_record_host(int32_t n, int32_t A, const float* logits, const int32_t* actions, const float* reward,
                           const uint8_t* terminated, const uint8_t* truncated, const float* terminal_value_or_null,
                           const double* episode_return_or_null, const int32_t* episode_length_or_null, double gamma,
                           float* log_prob, float* reward_out, uint8_t* start_next, int32_t* ep_count_or_null,
                           double* ep_return_sum_or_null, int32_t* ep_length_sum_or_null);
/* pe_logf of n host floats (tests measure it).  A function of its own: the selectors of
 * pe_policy_math_host stay 0..2, anything else PE_ERR_ARG as before. */
int pe_logf_host(int32_t n, const float* x, float* y);
/* pe_rollout_gae: rewards f32 (T rows), values f32 (T rows), starts u8 (T + 1 rows),
 * last_values f32[n]; advantages / returns f32 (T rows).  Row t of an array starts t * its
 * stride ELEMENTS after the pointer (reward_stride, value_stride, start_stride; out_stride
 * for both outputs); every stride >= n.  One thread per env, serial in t.  PE_ERR_ARG for
 * n < 1, T < 1, a stride < n or a NULL pointer. */
int pe_rollout_gae(int32_t T, int32_t n, int64_t reward_stride, int64_t value_stride, int64_t start_stride,
                   int64_t out_stride, const float* rewards, const float* values, const uint8_t* starts,
                   const float* last_values, double gamma, double gae_lambda, float* advantages, float* returns,
                   void* stream);
int pe_rollout_gae_host(int32_t T, int32_t n, int64_t reward_stride, int64_t value_stride, int64_t start_stride,
                        int64_t out_stride, const float* rewards, const float* values, const uint8_t* starts,
                        const float* last_values, double gamma, double gae_lambda, float* advantages, float* returns);

/* Replay collection: what SB3 2.2.1's OffPolicyAlgorithm.collect_rollouts, DQN.predict /
 * _sample_action, ReplayBuffer.add / sample and the target half of DQN.train add to the
 * act / step loop of a DQN (DQN("MlpPolicy", buffer_size=2000000, batch_size=64, gamma=0.99,
 * exploration_fraction=0.7, exploration_initial_eps=1.0, exploration_final_eps=0.05,
 * net_arch=[512,512,256]), trainingCode.py:203-247): epsilon-greedy exploration, the
 * transition ring with the terminal-observation and time-limit rules, uniform minibatch
 * sampling and the TD target.  The learner (loss, gradients, optimizer, polyak / hard update
 * of the target net) stays out of scope.  The functions work on caller-owned arrays; the
 * device ones run on the calling thread's current device, asynchronous on `stream`, with no
 * allocation and no sync (graph-capturable); the *_host twins execute the same definition on
 * host arrays and give the same bits (rl-env_amd/csrc/pe_replay_math.hpp).  Obs are byte
 * codes throughout (handles created with obs_codes; D = 5C + 27 bytes per obs): an f32 ring
 * is not provided.
 *
 * Control block: ctrl is a caller-owned DEVICE array of PE_REPLAY_CTRL_WORDS u64 words,
 * zeroed by the caller before the first call.  Word PE_RC_STEPS counts the rows of
 * transitions stored so far, word PE_RC_DRAWS the minibatches sampled so far; the rest is
 * reserved.  The counters live on the device so that a captured graph that is replayed
 * writes the next ring slot and draws fresh random numbers.  pe_replay_store and
 * pe_replay_sample advance their counter in a one-thread launch of its own behind the kernel
 * that reads it: no launch both reads a counter in many workgroups and advances it.
 * pe_replay_select only reads PE_RC_STEPS.
 *
 * Definition:
 *  - Random words of an event counter c (steps or draws), an index i and a domain word w:
 *    philox4x32-10(ctr = ((uint32)c, i, (uint32)(c >> 32), w), key = seed) -- (c, i, 0, w)
 *    for the first 2^32 events.  mulhi32(x, m) = (uint64)x * m >> 32.
 *  - select, per env e: (x, y, ..) = words(steps, env_id_offset + e, 0x53504545);
 *    u = (x >> 8) * 2^-24; the env explores iff u < eps, and then takes mulhi32(y, A) --
 *    uniform over all A actions, the greedy one included, as action_space.sample() --, else
 *    its greedy action.  eps = 0 reproduces the greedy actions, eps = 1 explores every env
 *    (SB3's learning_starts phase).  Exploration per env is this project's own definition:
 *    SB3's DQN.predict draws ONE np.random.rand() for the whole vector of envs, so that all
 *    envs explore or none does -- an artefact of small n_envs that is useless at 65536 envs --
 *    and numpy's generator is not reproduced.
 *  - store, one row of n transitions into ring slot steps % K, per env e: obs and action as
 *    given; reward as given; done = terminated (SB3's dones * (1 - timeouts), timeout =
 *    truncated && !terminated: an episode cut by the time limit alone still bootstraps);
 *    next_obs = the step's next obs where !(terminated | truncated), else the byte codes of
 *    the env's terminal obs (SB3's _store_transition: infos[i]["terminal_observation"]),
 *    encoded from the step's f32 terminal_obs row: column c < 5C: c % 5 == 0 -> rint(x R),
 *    else x != 0 ? R + 1 : 0; the two position columns 96 + rint(x G); the 25 visit columns
 *    80 + rint(10 x); products in f64, round-half-even (plantos_amd/codes.py encode_obs;
 *    expanding the code gives x back bit for bit).  Rows of terminal_obs of envs that are
 *    not done are never read.  A done env adds 1 to ep_count, episode_return to
 *    ep_return_sum and episode_length to ep_length_sum (per env, no atomics).  Then steps
 *    advances by 1.
 *  - sample, draw number `draws`, per sample j < B: filled = min(steps, K);
 *    (x, y, ..) = words(draws, j, 0x504D4153); slot = mulhi32(x, filled); env = mulhi32(y, n):
 *    uniform with replacement over what is stored, as ReplayBuffer.sample.  The outputs are
 *    the ring's rows at (slot, env) and the index pair.  With filled == 0 the indices are
 *    (-1, -1) and every other output row is zero.  Then draws advances by 1.
 *  - target, per sample j: g = (float)gamma; m = q_next[j][a*], a* the first maximum in action
 *    order; target = reward + (g * m) * (1 - (float)(done != 0)), every product and sum
 *    rounded on its own.
 *
 * Ring planes (caller-owned, device): obs / next_obs u8[K, n, D], actions i32[K, n], rewards
 * f32[K, n], dones u8[K, n].  PE_ERR_ARG with a message for sizes < 1, A outside 2..8, a NULL
 * required pointer, a geometry with D = 5C + 27 > 4096, and an output of pe_replay_sample or
 * a ring plane that is not 4-byte aligned. */
#define PE_REPLAY_CTRL_WORDS 4
enum pe_replay_ctrl { PE_RC_STEPS = 0, PE_RC_DRAWS = 1 };

/* greedy i32[n] (a forward's argmax actions), eps f32[1] (DEVICE: a schedule advances without
 * recapture), actions i32[n] (may be `greedy`), explored u8[n] or NULL (1 where the env
 * explored). */
int pe_replay_select(int32_t n, int32_t A, const int32_t* greedy, const float* eps, const uint64_t* ctrl,
                     uint64_t seed, uint32_t env_id_offset, int32_t* actions, uint8_t* explored_or_null,
                     void* stream);
int pe_replay_select_host(int32_t n, int32_t A, const int32_t* greedy, float eps, uint64_t steps, uint64_t seed,
                          uint32_t env_id_offset, int32_t* actions, uint8_t* explored_or_null);
/* obs u8[n, D] (the codes the policy acted on), actions i32[n], next_obs u8[n, D], reward
 * f32[n], terminated / truncated u8[n], terminal_obs f32[n, D] as pe_step_codes left them;
 * episode_return f64[n] / episode_length i32[n] or NULL; the accumulators may each be NULL.
 * There is no host twin: the definition is a copy plus the encoder (plantos_amd/replay.py
 * HostRing states it in numpy). */
int pe_replay_store(int32_t n, int32_t K, int32_t grid_size, int32_t lidar_range, int32_t lidar_channels,
                    const uint8_t* obs, const int32_t* actions, const uint8_t* next_obs, const float* reward,
                    const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs,
                    const double* episode_return_or_null, const int32_t* episode_length_or_null,
                    uint8_t* ring_obs, uint8_t* ring_next_obs, int32_t* ring_actions, float* ring_rewards,
                    uint8_t* ring_dones, int32_t* ep_count_or_null, double* ep_return_sum_or_null,
                    int32_t* ep_length_sum_or_null, uint64_t* ctrl, void* stream);
/* Outputs, dense: obs / next_obs u8[B, D], actions i32[B], rewards f32[B], dones u8[B],
 * indices i32[B, 2] = (slot, env).  Nothing past those extents is written. */
int pe_replay_sample(int32_t B, int32_t n, int32_t K, int32_t D, const uint8_t* ring_obs,
                     const uint8_t* ring_next_obs, const int32_t* ring_actions, const float* ring_rewards,
                     const uint8_t* ring_dones, uint64_t seed, uint64_t* ctrl, uint8_t* obs, uint8_t* next_obs,
                     int32_t* actions, float* rewards, uint8_t* dones, int32_t* indices, void* stream);
/* The indices pe_replay_sample draws with the counters at (steps, draws); the gather itself
 * is a copy. */
int pe_replay_sample_indices_host(int32_t B, int32_t n, int32_t K, uint64_t steps, uint64_t draws, uint64_t seed,
                                  int32_t* indices);
/* q_next f32[B, A] (the target network's Q-values of next_obs), rewards f32[B], dones u8[B];
 * targets f32[B]. */
int pe_replay_target(int32_t B, int32_t A, const float* q_next, const float* rewards, const uint8_t* dones,
                     double gamma, float* targets, void* stream);
int pe_replay_target_host(int32_t B, int32_t A, const float* q_next, const float* rewards, const uint8_t* dones,
                          double gamma, float* targets);

/* Introspection for tests / benchmarks. */
int32_t pe_num_envs(const pe_handle* h);
int32_t pe_kernel_variant(const pe_handle* h);  /* 0 generic, >0 specialized geometry */
const char* pe_kernel_name(const pe_handle* h);
int32_t pe_prefetch_every(const pe_handle* h);  /* steps between prefetch launches, 0 = off */
uint64_t pe_state_bytes(const pe_handle* h);

const char* pe_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
