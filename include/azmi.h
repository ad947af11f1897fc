/* azmi.h — C ABI of the MI355X-native self-play engine (libazmi.so).
 *
 * Drop-in boundary for the reference's PlayManager/MCTS hot path.  Every entry
 * point below replaces one member of the reference's pybind11 surface
 * (/root/reference/src/py_wrapper.cc) or of the C++ class behind it; the
 * reference file:line each one stands in for is cited next to it.  Plain
 * pointers and sizes only: no torch, pybind11 or HIP types cross this line
 * (`stream` is a hipStream_t passed as void*; `dev_*` pointers are HIP device
 * addresses, e.g. torch.Tensor.data_ptr()).
 *
 * All functions return 0 on success or a negative azmi_status; the message of
 * the last error on the calling thread is available from azmi_last_error().
 * The library has NO CPU fallback: without a HIP device azmi_pm_create fails
 * with AZMI_ERR_NO_DEVICE.
 */
#ifndef AZMI_H_
#define AZMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZMI_ABI_VERSION 1

typedef enum azmi_status {
  AZMI_OK = 0,
  AZMI_ERR_INVALID = -1,   /* bad argument (reference: std::runtime_error -> RuntimeError) */
  AZMI_ERR_NO_DEVICE = -2, /* no HIP device / HIP runtime error */
  AZMI_ERR_OOM = -3,
  AZMI_ERR_OVERFLOW = -4,  /* a device-side arena / history ring ran out of room */
  AZMI_ERR_STATE = -5,
  AZMI_ERR_RANGE = -6      /* index out of range (reference: std::out_of_range -> IndexError) */
} azmi_status;

/* game ids (reference GAME_REGISTRY, config.py:17-35) */
typedef enum azmi_game { AZMI_GAME_CONNECT4 = 0, AZMI_GAME_TAWLBWRDD = 1, AZMI_GAME_BRANDUBH = 2, AZMI_GAME_OPENTAFL = 3,
                         /* StarGambitUnifiedGS (star_gambit_gs.h:788-887): four variants on the 13 x 13 canvas, 36 planes, 1709 moves,
                          * relative values, several actions per turn */
                         AZMI_GAME_STARGAMBIT = 4 } azmi_game;

/* EvalType, play_manager.h:20 */
typedef enum azmi_eval_type { AZMI_EVAL_NN = 0, AZMI_EVAL_RANDOM = 1, AZMI_EVAL_PLAYOUT = 2 } azmi_eval_type;

#define AZMI_MAX_PLAYERS 4
#define AZMI_MAX_PERMS 8    /* seat permutations (2 players: 2; the reference cycles or enumerates them, game_runner.py:2208-2231) */
#define AZMI_MAX_GROUPS 4   /* model groups = distinct networks in one PlayManager */

/* POD mirror of struct PlayParams (play_manager.h:60-154): same names, same
 * meaning, same defaults (azmi_play_params_default).  Vectors become fixed
 * arrays + a count. */
typedef struct azmi_play_params {
  uint32_t games_to_play;
  uint32_t concurrent_games;
  uint32_t max_batch_size;
  uint32_t max_cache_size;
  uint32_t cache_shards;
  uint32_t num_mcts_visits;                 /* must equal num_players (play_manager.cc:20-22) */
  uint32_t mcts_visits[AZMI_MAX_PLAYERS];
  float cpuct;
  float start_temp;
  float final_temp;
  float temp_decay_half_life;
  int32_t history_enabled;
  int32_t self_play;
  int32_t tree_reuse;
  float epsilon;
  float mcts_root_temp;
  int32_t playout_cap_randomization;
  uint32_t playout_cap_depth;
  float playout_cap_percent;
  float fpu_reduction;
  int32_t root_fpu_zero;
  int32_t shaped_dirichlet;
  int32_t policy_target_pruning;
  float resign_percent;
  float resign_playthrough_percent;
  uint32_t num_eval_type;                   /* 0 = all NN */
  int32_t eval_type[AZMI_MAX_PLAYERS];
  /* Gumbel AlphaZero (play_manager.h:103-116; mcts.cc:24-401): full searches use Gumbel-Top-k +
   * sequential halving at the root, the improved policy as the training target and the
   * deterministic final action; capped searches stay PUCT unless fast_search_uses_gumbel. */
  int32_t gumbel_enabled;
  uint32_t gumbel_m;                        /* default 16, at most 64 here */
  float gumbel_c_visit;                     /* default 50 */
  float gumbel_c_scale;                     /* default 1 */
  int32_t gumbel_full;
  int32_t fast_search_uses_gumbel;
  /* model groups and seat permutations (play_manager.h:118-154; normalised as play_manager.cc:24-113 does):
   * model_groups[player] = network index (0 entries = identity, i.e. one group per player);
   * seat_perms[perm][seat] = model group sitting in that seat for games with perm_index == perm
   * (0 perms = one permutation equal to model_groups); game i starts with perm i % num_seat_perms.
   * mcts_visits / eval_type are per PLAYER and become per-group (last player of a group wins), then per seat. */
  uint32_t num_model_groups_given;
  uint8_t model_groups[AZMI_MAX_PLAYERS];
  uint32_t num_seat_perms;
  uint8_t seat_perms[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  /* per-permutation x per-seat overrides [num_seat_perms][num_players]; has_* = 0 -> filled from the globals */
  int32_t has_seat_visits, has_seat_cap_visits, has_seat_epsilon, has_seat_mcts_root_temp, has_seat_root_fpu_zero;
  uint32_t seat_visits[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  uint32_t seat_cap_visits[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  float seat_epsilon[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  float seat_mcts_root_temp[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  uint8_t seat_root_fpu_zero[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  /* per-seat Gumbel and resign overrides, play_manager.h:126-153 / play_manager.cc:116-176 (same has_* convention; defaults:
   * the global gumbel_* fields, use_improved_policy 0, resign threshold -2 = off, consecutive 1) */
  int32_t has_seat_gumbel_enabled, has_seat_gumbel_m, has_seat_gumbel_c_visit, has_seat_gumbel_c_scale, has_seat_gumbel_full,
          has_seat_gumbel_use_improved_policy, has_seat_resign_threshold, has_seat_resign_consecutive;
  uint8_t seat_gumbel_enabled[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  uint8_t seat_gumbel_full[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  uint8_t seat_gumbel_use_improved_policy[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  uint32_t seat_gumbel_m[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  uint32_t seat_resign_consecutive[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  float seat_gumbel_c_visit[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  float seat_gumbel_c_scale[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  float seat_resign_threshold[AZMI_MAX_PERMS][AZMI_MAX_PLAYERS];
  /* temp_decay_half_life_by_variant (play_manager.h:87-90, play_manager.cc:290-296): entry get_variant_id() replaces
   * temp_decay_half_life when it exists; games without variants (id -1) ignore it */
  uint32_t num_temp_decay_half_life_by_variant;
  float temp_decay_half_life_by_variant[4];
} azmi_play_params;

/* engine-only knobs that have no reference counterpart */
typedef struct azmi_engine_opts {
  uint64_t seed;          /* slot s uses pcg32 stream slot_seed(seed, s) */
  int32_t device;         /* HIP device ordinal */
  uint32_t max_inline;    /* simulations a slot may finish inside one round without the net
                             (terminal leaves, RANDOM eval, cache hits); 0 = default */
  uint32_t history_capacity; /* rows of the device history buffer; 0 = sized from params */
  int32_t log_moves;      /* keep a per-move log (parity tests) */
  uint32_t move_log_capacity;
  /* the base GameState of PlayManager(gs, params) where it has constructor arguments: StarGambitUnifiedGS(pinned_variant,
   * probs) (py_wrapper.cc:662-667; defaults -1 and four times 0.25).  Every new game draws its variant from the slot's coin
   * stream unless pinned (build-defined draw: the reference's engine is unseedable, star_gambit_gs.cc:2357-2362) */
  int32_t sg_pinned_variant;
  float sg_variant_probs[4];
} azmi_engine_opts;

typedef struct azmi_pm azmi_pm;

/* `stream` arguments are hipStream_t values used as given (NULL is the HIP null stream);
 * AZMI_STREAM_ENGINE selects the engine's own non-blocking stream. Result queries order
 * themselves behind the stream of the most recent round/play/poll call. */
#define AZMI_STREAM_ENGINE ((void*)(intptr_t)-1)

void azmi_play_params_default(azmi_play_params* p);      /* PlayParams{} defaults, play_manager.h:60-154 */
void azmi_engine_opts_default(azmi_engine_opts* o);
const char* azmi_last_error(void);
int azmi_abi_version(void);
int azmi_device_count(void);

/* static game facts: GameState::num_moves/num_players + CANONICAL_SHAPE (py_wrapper.cc:157-189, 562-580) */
int azmi_game_info(int game, uint32_t* num_players, uint32_t* num_moves, uint32_t chw[3]);

/* PlayManager(gs, params) — py_wrapper.cc:352-354, play_manager.cc:12-256 */
int azmi_pm_create(int game, const azmi_play_params* params, const azmi_engine_opts* opts, azmi_pm** out);
/* PlayManager(gs, params, caches) — py_wrapper.cc:355-360, play_manager.cc:644-649: params.max_cache_size is ignored and model
 * group g uses caches[g] (an azmi_cache from azmi_cache_create, see below; NULL entries = no cache for that group).  The
 * caches are not owned: they must outlive the engine, and they keep their contents from one engine to the next.  The engine
 * probes 64-entry shards, so a cache must have been created with shards = max_size / 64. */
typedef struct azmi_cache azmi_cache;
int azmi_pm_create_with_caches(int game, const azmi_play_params* params, const azmi_engine_opts* opts, azmi_cache* const* caches,
                               uint32_t num_caches, azmi_pm** out);
void azmi_pm_destroy(azmi_pm* pm);

/* ---- device fast path (what PlayManager::play + GameRunner's batcher/result_worker do,
 *      play_manager.cc:258-600 + game_runner.py:651-726, without leaving HBM) ---------------
 * One round = every live slot: consume its (v, pi) row -> backup -> maybe play a move ->
 * descend to the next leaf -> write that leaf's canonical planes into row `slot` of the
 * leaf batch.  Rows are slot-indexed, so the batch shape is always
 * [concurrent_games, C, H, W] and a round needs no host round-trip. */
int azmi_pm_round(azmi_pm* pm, void* stream);
/* device pointers of the slot-indexed buffers: canonical [S,C,H,W] (engine writes, net reads),
 * v [S,P+1] and pi [S,M] (net writes probabilities, engine reads) — replaces
 * build_batch / update_inferences, py_wrapper.cc:449-504 / play_manager.cc:619-642 */
int azmi_pm_io_buffers(azmi_pm* pm, float** dev_canonical, float** dev_v, float** dev_pi);
/* play() for EvalType::RANDOM on every seat: rounds until games_completed >= games_to_play */
int azmi_pm_play(azmi_pm* pm, void* stream);
/* copies the small control block back (sync on `stream`); mirrors remaining_games()/games_completed() */
int azmi_pm_poll(azmi_pm* pm, void* stream, uint32_t* games_completed, uint32_t* live_slots);

/* stop() / stopped(), play_manager.h:177-178: play() and build_batch return at their next check; may be called from another thread */
int azmi_pm_stop(azmi_pm* pm);
int azmi_pm_stopped(azmi_pm* pm, int* out);
/* awaiting_inference_count() / awaiting_mcts_count(), play_manager.h:316-323 */
int azmi_pm_queue_counts(azmi_pm* pm, uint32_t* awaiting_inference, uint32_t* awaiting_mcts);
/* game_data(i).gs, play_manager.h:286: the packed state of the game in slot i.  Connect4: words = {stones of player 0, stones
 * of player 1 (bit h*7+w), turn | player << 32}; Tafl family: {defenders lo, hi, attackers lo, hi (bit = square),
 * king square | turn << 8 | player << 24 | repetition count << 32}; one more word follows: GameData::perm_index, the seat
 * permutation the slot's game runs under (play_manager.h:41).  `cap` >= state words + 1.  AZMI_ERR_RANGE for a bad index. */
int azmi_pm_slot_state(azmi_pm* pm, uint32_t slot, uint64_t* words, uint32_t cap, uint32_t* n);
/* StarGambit: state words = 20 packed units (two per word: type 0:2 | player 2 | slot 3:3 | hp 6:3 | facing 9:3 | q+6 12:4 |
 * r+6 16:4 | moves_left 20:2 | cannons_fired 22:4 | exists 26) + one word player | turn << 8 | misc << 24 (units 0:5, acted 5, over 6,
 * winner 7:2, variant 9:2) | reserves << 40 (3 bits per [player][type]); its position history (star_gambit_gs.h:745) comes
 * from azmi_pm_slot_history: the slot's entries since the last deploy (the reference's own position hashes); 0 entries for Connect4 */
int azmi_pm_slot_history(azmi_pm* pm, uint32_t slot, uint64_t* out, uint32_t cap, uint32_t* n);
/* game_data(i).canonical(), py_wrapper.cc:279-288: the leaf planes slot i is waiting on, to a HOST array [C,H,W] */
int azmi_pm_slot_canonical(azmi_pm* pm, uint32_t slot, float* out);

/* ---- results (all synchronise on the engine's stream first) -------------------------------- */
int azmi_pm_scores(azmi_pm* pm, float* out /* [P+1] */);          /* scores(), play_manager.h:173 */
int azmi_pm_resign_scores(azmi_pm* pm, float* out /* [P+1] */);   /* resign_scores(), :174 */
/* out[7] = avg_game_length, avg_leaf_depth, avg_search_entropy, fast_avg_leaf_depth,
 *          fast_avg_search_entropy, avg_moves_per_turn, avg_valid_moves (play_manager.h:288-315) */
int azmi_pm_stats(azmi_pm* pm, float* out);
/* the sums behind those averages, to combine several engines (shards of one GPU, ranks) exactly: out[10] = sum of game
 * lengths, games completed, total / full / fast move counts, sums of leaf depth, search entropy, fast leaf depth, fast
 * entropy, valid moves (play_manager.h:398-424) */
int azmi_pm_stat_sums(azmi_pm* pm, double* out);
/* out[6] = simulations, leaf evaluations requested from the net, cache hits, cache misses,
 *          history rows available, rounds */
int azmi_pm_counters(azmi_pm* pm, uint64_t* out);
/* out[6] = cache_hits, cache_misses, cache_evictions, cache_reinserts, cache_size, cache_max_size summed over the model
 *          groups' caches (play_manager.h:325-366) */
int azmi_pm_cache_stats(azmi_pm* pm, uint64_t out[6]);
/* build_history_batch, py_wrapper.cc:393-424: copies up to `cap` finished rows to HOST arrays
 * canonical [cap,C,H,W], v [cap,P+1], pi [cap,M]; returns rows written in *n */
int azmi_pm_pop_history(azmi_pm* pm, float* canonical, float* v, float* pi, uint32_t cap, uint32_t* n);
/* same rows, left in HBM: device pointers + row count (for the RCCL sample gather) */
int azmi_pm_history_device(azmi_pm* pm, float** dev_canonical, float** dev_v, float** dev_pi,
                           uint32_t** dev_meta, uint32_t* rows);
/* The finished-sample store is a RING of `capacity` rows (the reference's history queue is unbounded and drained by
 * GameRunner.hist_saver, game_runner.py:729-747): the unread rows are `rows` rows starting at physical row `first_row`
 * of the azmi_pm_history_device arrays, wrapping modulo `capacity`.  azmi_pm_history_consume releases the oldest `rows`
 * unread rows (azmi_pm_pop_history does both for host arrays).  The engine stops with AZMI_ERR_OVERFLOW (mask 2) when a
 * finished game finds less room than its rows. */
int azmi_pm_history_window(azmi_pm* pm, uint32_t* first_row, uint32_t* rows, uint32_t* capacity);
int azmi_pm_history_consume(azmi_pm* pm, uint32_t rows);
/* per-move log (opts.log_moves): rows [n,8] = slot, game_in_slot, move, turn, player, capped,
 * pcg32 state (lo, hi) of the slot's tree stream right before pick_move's draw;
 * counts [n,M] = root counts() right before the move.  Parity-test hook. */
int azmi_pm_move_log(azmi_pm* pm, uint32_t* rows, uint32_t* counts, uint32_t cap, uint32_t* n);
/* games each slot has completed, [S] */
int azmi_pm_slot_games(azmi_pm* pm, uint32_t* out);

/* ---- host-buffer compatibility path (exact reference signatures) ---------------------------
 * build_batch(group, batch) — py_wrapper.cc:449-504: runs rounds until a leaf batch is
 * pending, copies the live rows to the HOST array batch[cap,C,H,W], returns their slot ids.
 * batch == NULL hands out the indices only: pop_game / pop_games_upto (play_manager.h:186-192). */
int azmi_pm_build_batch(azmi_pm* pm, float* batch, uint32_t cap, uint32_t* indices, uint32_t* n);
/* update_inferences(group, indices, v, pi) — play_manager.cc:619-642, HOST arrays */
int azmi_pm_update_inferences(azmi_pm* pm, const uint32_t* indices, uint32_t n, const float* v, const float* pi);

/* per-variant tables of a game with variants (play_manager.h:218-275; play_manager.cc:237-255, 468-484).
 * azmi_pm_num_variants: num_tracked_variants().  azmi_pm_variant_sums(v): perm_scores [perms][P+1] (variant_perm_scores; their
 * sum over perms = variant_scores), perm_games [perms], sums[10] = game_length, games, total / full / fast move counts, leaf
 * depth, entropy, fast leaf depth, fast entropy, valid moves - the accumulators behind the variant_avg_* getters */
uint32_t azmi_pm_num_variants(azmi_pm* pm);
int azmi_pm_variant_sums(azmi_pm* pm, uint32_t variant, float* perm_scores, uint32_t* perm_games, double* sums);

/* ---- GameState / MCTS single-object surface on the device (py_wrapper.cc:157-220) ----------
 * Batched over `n` independent states so one launch covers many objects. Used by the
 * parity tests of the rules kernels (SURVEY tier T0). `moves` is [n, len] row-major; a
 * negative entry stops that game early.  Outputs (any may be NULL):
 *   valid [n,M] u8, scores [n,P+1] f32 (all -1 if not over), canonical [n,C,H,W] f32,
 *   player [n] u32, turn [n] u32, key [n] u64, status [n] i32 (0 ok, -1 illegal move). */
int azmi_game_replay(int game, int device, const int32_t* moves, uint32_t n, uint32_t len,
                     uint8_t* valid, float* scores, float* canonical, uint32_t* player,
                     uint32_t* turn, uint64_t* key, int32_t* status);
/* the same from given start positions: `init` is [n, init_stride] bytes, one serialized state per
 * game in the reference's pickle image (Connect4GS::to_bytes, connect4_gs.cc:172-190: int8
 * board[2][6][7], int8 player, int32 turn = 89 bytes; Connect4GS(board, player, turn) ctor,
 * py_wrapper.cc:563-581).  Brandubh / OpenTafl: int8 board[3][N][N] (king, defenders, attackers), int8 player,
 * int32 turn = 3*N*N + 5 bytes, with an empty repetition map (the reference tests' MakeGS helper,
 * opentafl_gs_test.cc:97-101).  StarGambit: StarGambitUnifiedGS::to_bytes (star_gambit_gs.cc:2446-2449 around the inner image
 * :2246-2251), any length up to init_stride, rows padded with zeros; its replay/playout kernels take one wavefront per game.
 * NULL = the game's initial position (StarGambit: the Skirmish variant). */
int azmi_game_replay_from(int game, int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves,
                          uint32_t n, uint32_t len, uint8_t* valid, float* scores, float* canonical,
                          uint32_t* player, uint32_t* turn, uint64_t* key, int32_t* status);
/* playout_eval(gs) / playout_eval_batch(states), game_state.cc:10-95 (Python: py_wrapper.cc:726-770): for each of n states
 * (start position + move list, as in azmi_game_replay_from) pi = uniform over the legal moves, v = the scores of a uniformly
 * random rollout.  The reference's rollout RNG is an unseedable thread-local engine; here state i uses a pcg32 stream
 * seeded with seeds[i].  v [n,P+1], pi [n,M] are HOST arrays.  All five games; EvalType::PLAYOUT seats of an engine run the same
 * rollout on the device from the slot's third pcg32 stream. */
int azmi_playout_eval(int game, int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                      const uint64_t* seeds, float* v, float* pi);
/* flags bit 0 (Brandubh / OpenTafl): apply moves the way the reference's play_move does — no ownership or slide
 * check, captures judged from the moved piece's side (brandubh_gs.cc:342-427; the reference's own tests rely on
 * it).  Without the flag a move that valid_moves() does not list ends the game record with status -1. */
int azmi_game_replay_ex(int game, int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves,
                        uint32_t n, uint32_t len, uint8_t* valid, float* scores, float* canonical,
                        uint32_t* player, uint32_t* turn, uint64_t* key, int32_t* status, uint32_t flags);

/* StarGambitUnifiedGS::to_bytes (star_gambit_gs.cc:2451-2465; py::pickle of the game objects, py_wrapper.cc:77-83) of n
 * states given as start image + moves (as azmi_game_replay_from; flags as azmi_game_replay_ex): out [n, out_stride] bytes,
 * out_len [n] image sizes, status [n] (0 ok, -1 illegal move / malformed start, -2 image longer than out_stride).  The
 * variant_probs / pinned_variant fields of the header (bytes 0-19) are left zero: they are constructor arguments the caller keeps. */
int azmi_sg_image(int device, const uint8_t* init, uint32_t init_stride, const int32_t* moves, uint32_t n, uint32_t len,
                  uint8_t* out, uint32_t out_stride, uint32_t* out_len, int32_t* status, uint32_t flags);

/* ---- training-sample symmetries (GameState::symmetries(PlayHistory), py_wrapper.cc:178;
 *      connect4_gs.cc:151-170, tafl_helper.h:16-149, tawlbwrdd_gs.cc:455-458) ------------------
 * `count` samples in: canon [count,C,H,W], v [count,P+1], pi [count,M]; out: the NUM_SYMMETRIES
 * images of every sample, sample-major, in the reference's order (Connect4 {base, mirror}; Tafl
 * {base, r, r^2, r^3, m(base), m(r), m(r^2), m(r^3)}): out_canon [count,NS,C,H,W], out_v
 * [count,NS,P+1], out_pi [count,NS,M].  Pointers are DEVICE pointers (asynchronous on `stream`)
 * unless host_buffers != 0 (then HOST arrays, staged through HBM, synchronous). */
uint32_t azmi_num_symmetries(int game);
int azmi_symmetries(int game, int device, uint32_t count, const float* canon, const float* v, const float* pi,
                    float* out_canon, float* out_v, float* out_pi, int host_buffers, void* stream);
/* the same for any square Tafl board (Brandubh 7, Tawlbwrdd 11, OpenTafl 11 share tafl_helper.h) */
int azmi_tafl_symmetries(uint32_t board, uint32_t channels, uint32_t num_values, int device, uint32_t count,
                         const float* canon, const float* v, const float* pi, float* out_canon, float* out_v,
                         float* out_pi, int host_buffers, void* stream);
const char* azmi_symmetries_last_error(void);

/* ---- per-row surprise loss and resample_by_surprise on the device (game_runner.py:1148-1255; sample_loss / sample_loss_pi /
 *      sample_loss_v, neural_net.py:664-676, 875-879; csrc/samples_kernels.h).  Everything in float64 on the float32
 *      inputs.  `dev_*` are DEVICE pointers; `stream` is a HIP stream or NULL; the message of a failed call is in
 *      azmi_samples_last_error().  n == 0 is legal everywhere and touches no device; n > 2^30 is AZMI_ERR_INVALID.
 *   sample_loss      dev_loss_out[i] = -scale * sum over m with target[i,m] > 0, of target[i,m] * log(max(p[i,m], FLT_MIN)), for two
 *                    [n, M] float32 arrays, p holding PROBABILITIES (what azmi_net_forward writes; the reference's outputs are
 *                    log-probabilities): sample_loss_pi at scale = 1, sample_loss_v at scale = cv.  A zero target contributes
 *                    exactly 0 whatever p is; a negative target makes the row NaN.  A row's bits do not depend on n.  One launch,
 *                    asynchronous.  M == 0 or M > 2^20 is AZMI_ERR_INVALID.
 *   resample_plan    from dev_loss [n] f64: total_loss (a tree sum whose order is fixed by n alone: the same bits on every run and
 *                    stream), nonfinite / first_nonfinite (the number of rows that are NaN or +-inf and the first of them,
 *                    0xFFFFFFFF for none), and - unless dev_copies and dev_offsets are both NULL, which leaves the sums alone -
 *                    dev_copies [n] u32, dev_offsets [n] u64 = the exclusive prefix sum of the copies, rows_out = their sum.
 *                    total_loss <= 0: every count is 1.  Otherwise, every operation in float64 in this order:
 *                      w = 0.5 + (loss[i] / total_loss) * 0.5 * n,  k = floor(w),  copies[i] = k + (u_i < w - k)
 *                      u_i = (mix64(seed + 0x9E3779B97F4A7C15 * (i + 1)) >> 11) * 2^-53      (mix64: csrc/dev_rng.h; mod 2^64)
 *                    (the weights and the rounding rule of game_runner.py:1189-1193; the draw is ours: the reference's comes from
 *                    the global numpy state).  With nonfinite > 0 the counts are unspecified (each is a valid u32, their sum is
 *                    rows_out).  Synchronises `stream` once, to hand back the record; the scratch block is kept per device between
 *                    calls (no allocation in the steady state).  The thread's current device is left as it was (all three).
 *   resample_gather  out[offsets[i] + c] = in[i] for c < copies[i], for the n_arrays <= 8 row arrays dev_in[k] -> dev_out[k] with
 *                    rows of row_bytes[k] bytes (whole dwords; dev_in, dev_out, row_bytes are HOST arrays of n_arrays entries):
 *                    x[np.repeat(np.arange(n), copies)].  dev_out[k] has room for rows_out rows.  Rows whose size and both base
 *                    addresses are multiples of 16 move as 16-byte accesses, the others as dwords.  One launch, asynchronous. */
typedef struct azmi_resample_record {
  double total_loss;
  uint64_t rows_out;
  uint32_t nonfinite;
  uint32_t first_nonfinite;
} azmi_resample_record;
int azmi_sample_loss(const float* dev_target, const float* dev_p, uint32_t n, uint32_t M, double scale, double* dev_loss_out, int device,
                     void* stream);
int azmi_resample_plan(const double* dev_loss, uint32_t n, uint64_t seed, uint32_t* dev_copies, uint64_t* dev_offsets,
                       azmi_resample_record* host_record_out, int device, void* stream);
int azmi_resample_gather(const uint32_t* dev_copies, const uint64_t* dev_offsets, uint32_t n, uint32_t n_arrays, const void* const* dev_in,
                         void* const* dev_out, const uint32_t* row_bytes, int device, void* stream);
const char* azmi_samples_last_error(void);

/* ---- per-row policy and value diagnostics of a net against the samples, and their bucketed sums (network_pareto.eval_loss,
 *      network_pareto.py:652-738; _analyze_iteration_variants, game_runner.py:2509-2627; csrc/sample_metrics_kernels.h, DESIGN.md
 *      §8.5).  The conventions of the block above: float64 on the float32 inputs, DEVICE pointers, `stream` a HIP stream or NULL,
 *      the message of a failed call in azmi_samples_last_error(), argument errors are AZMI_ERR_INVALID before any device call,
 *      n == 0 is legal and touches no device, n <= 2^30, 1 <= M, V <= 2^20, the thread's current device is left as it was.
 *   sample_metrics   one launch over target_pi / p_pi [n, M] and target_v / p_v [n, V] (p: PROBABILITIES), every element read
 *                    once.  Per row i it writes the 13 float64 columns dev_cols_out[c * col_stride + i] (col_stride >= n; c:
 *                    SampleMetric of csrc/sample_metrics_kernels.h = alphazero.samples.Metric) and two u32:
 *                       0 pi_loss         -sum over t > 0 of t * log(max(p, FLT_MIN))      = azmi_sample_loss at scale 1, bit for bit
 *                       1 v_loss          the same on the value rows, times cv             = azmi_sample_loss at scale cv, bit for bit
 *                       2 target_entropy  -sum over t > 0 of t * log(t)
 *                       3 entropy         -sum over all m of t * log(t + 1e-9)
 *                       4 kl              sum over t > 0 of t * log(t / (p + 1e-10))
 *                       5 top1            max_m t            6 net_top1     max_m p        7 net_at_mcts  p[mcts_argmax]
 *                       8 top1_gap        top1 - net_at_mcts 9 top1_agree   1.0 when net_argmax == mcts_argmax, else 0.0
 *                      10 top3_overlap    |top3(p) & top3(t)|, 0..3 (M < 3: the sets have M members)
 *                      11 v_pred          p_v[i, 0]         12 v_actual     target_v[i, 0]
 *                      dev_mcts_argmax_out[i], dev_net_argmax_out[i]: the argmax of the target and of the net's row.
 *                    Ties in every argmax and top-3 go to the LOWER index (np.argmax, a stable argsort of -x) - NOT the rule of
 *                    azmi_policy_divergences / sweep_metrics, where the higher index wins.  A negative target makes the sums of
 *                    its row NaN (policy: columns 0, 2, 3, 4; value: column 1); a NaN probability makes NaN what reads it
 *                    (pi_loss and kl under a positive target, net_top1 anywhere in the row, net_at_mcts and top1_gap at the
 *                    target's argmax); the index columns of such a row are unspecified but < M.  A row's bits do not depend on n.
 *   sample_plane_argmax  dev_out[i] (u8) = the lower-index argmax over the planes first_plane .. first_plane + n_planes - 1
 *                    (1 <= n_planes <= 16, inside C) of dev_canonical [n, C, H, W] at cell (row, col): the variant id of the
 *                    unified StarGambit encoding is (32, 4, 6, 6).  One launch, asynchronous.
 *   sample_metrics_reduce  sum[b][c] = the float64 sum of column c over the rows with dev_bucket[i] == b (u8 [n]; NULL with
 *                    n_buckets == 1: every row is in bucket 0), 1 <= n_buckets <= 8, count[b] the rows of bucket b, total[c] the sum
 *                    over every row.  The tile tree of resample_plan (tiles of 1024, a row outside the bucket enters as +0.0): the
 *                    bits of a sum depend on n and on which rows belong, on nothing else.  nonfinite / first_nonfinite: the rows
 *                    with a NaN or +-inf in one of the columns 0..4 and the first of them (0xFFFFFFFF for none); invalid: the rows
 *                    whose id is >= n_buckets, which belong to no bucket (total[] holds them).  One launch per level (at most
 *                    three); synchronises `stream` once, to hand back the record; the scratch block is kept per device. */
#define AZMI_SAMPLE_METRIC_COLUMNS 13
#define AZMI_SAMPLE_METRIC_MAX_BUCKETS 8
typedef struct azmi_sample_metrics_record {
  double sum[AZMI_SAMPLE_METRIC_MAX_BUCKETS][AZMI_SAMPLE_METRIC_COLUMNS];
  double total[AZMI_SAMPLE_METRIC_COLUMNS];
  uint32_t count[AZMI_SAMPLE_METRIC_MAX_BUCKETS];
  uint32_t nonfinite;
  uint32_t first_nonfinite;
  uint32_t invalid;
  uint32_t reserved;
} azmi_sample_metrics_record;
int azmi_sample_metrics(const float* dev_target_pi, const float* dev_p_pi, const float* dev_target_v, const float* dev_p_v, uint32_t n,
                        uint32_t M, uint32_t V, double cv, double* dev_cols_out, uint64_t col_stride, uint32_t* dev_mcts_argmax_out,
                        uint32_t* dev_net_argmax_out, int device, void* stream);
int azmi_sample_plane_argmax(const float* dev_canonical, uint32_t n, uint32_t C, uint32_t H, uint32_t W, uint32_t first_plane,
                             uint32_t n_planes, uint32_t row, uint32_t col, uint8_t* dev_out, int device, void* stream);
int azmi_sample_metrics_reduce(const double* dev_cols, uint64_t col_stride, uint32_t n, const uint8_t* dev_bucket, uint32_t n_buckets,
                               azmi_sample_metrics_record* host_record_out, int device, void* stream);

/* ---- the history window and the recency-weighted reservoir on the device (csrc/samples_window_kernels.h).  The
 *      conventions of the two blocks above: DEVICE pointers, `stream` a HIP stream or NULL, the message of a failed call in
 *      azmi_samples_last_error(), argument errors are AZMI_ERR_INVALID before any device call, at most 2^30 rows per call, an empty
 *      call touches no device, the thread's current device is left as it was.
 *   samples_reservoir_keys  replaces `ages = (iteration - pool_iters).clamp(min=0); weights = decay ** ages` and the draw of
 *                    torch.multinomial(weights, k, replacement=False) (game_runner.py:1845-1849): dev_keys_out[i] (f64) =
 *                      log(u_i) / w_i,   w_i = decay ** max(0, iteration - dev_iters[i])   (dev_iters: i32 [n])
 *                      u_i = m_i * 2^-53,  m_i = ((mix64(seed + 0x9E3779B97F4A7C15 * (id_i + 1)) >> 12) << 1) | 1   (mod 2^64)
 *                    id_i = dev_row_ids[i] (u64 [n]) or i when that is NULL.  u_i is strictly inside (0, 1), so a key is negative
 *                    and finite unless w_i underflows to 0, which gives -inf; decay == 1 gives log(u_i).  The k LARGEST keys are a
 *                    sample of k rows without replacement with probabilities proportional to w (successive sampling: the
 *                    distribution of torch.multinomial, not its stream).  dev_bits_out (u64 [n], may be NULL) receives m_i.
 *                    decay outside (0, 1] or a non-finite iteration is AZMI_ERR_INVALID.  One launch, asynchronous.
 *   samples_select_top  replaces the selection of torch.multinomial and the fancy index `pool[selected]` it feeds
 *                    (game_runner.py:1847-1855): dev_index_out (i64 [k]) = the rows of the k largest of the n f64 keys, in
 *                    ASCENDING ROW ORDER; among equal keys the lower rows win; -0.0 counts as +0.0; -inf loses to every finite
 *                    key.  A radix select over the order-preserving 64-bit image of the keys (8 histogram passes of 8 bits) and an
 *                    ordered compaction: no sort, and a result that does not depend on scheduling.  The record: selected (= k),
 *                    threshold_key (the smallest chosen key), nan_rows / first_bad_row (the rows that are NaN and the first of
 *                    them, 0xFFFFFFFF for none; with a NaN the index list is unspecified but every entry is < n).  k > n is
 *                    AZMI_ERR_INVALID; k == 0 touches no device.  Synchronises `stream` once, to hand back the record; the scratch
 *                    block is kept per device.
 *   samples_window_gather  replaces the shuffled, cross-file-mixed pass of StreamingCompressedDataset (game_runner.py:1923-2009) that
 *                    train() cuts into batches (game_runner.py:1289-1345), and the row gather of update_reservoir:
 *                      out[j] = window[p],  p = perm(first + j),  j < rows
 *                    over a window of n_segments <= 64 arrays dev_segments[s] of segment_rows[s] rows (HOST arrays; a segment may
 *                    be empty) of row_bytes bytes (whole dwords, < 64 MiB), read as their concatenation; total <= 2^40 rows,
 *                    first + rows <= total.  perm is a bijection of [0, total) computed per row, no table and no sort: a Feistel
 *                    network of 6 rounds over b = max(2, ceil(log2 total)) bits, halves of b / 2 and b - b / 2 bits that swap every
 *                    round, x = (R << wl) | (L ^ (mix64(R + key_r) & (2^wl - 1))), key_r = mix64(k0 + 0x9E3779B97F4A7C15 * (r + 1)),
 *                    k0 = mix64(seed + 0x9E3779B97F4A7C15 * (pass_index + 1)), repeated until the value is < total.  With dev_index
 *                    (i64, at least first + rows entries) p = dev_index[first + j] instead (an entry outside the window reads its
 *                    last row).  Rows move as 16-byte accesses when row_bytes and every base address are multiples of 16, as
 *                    dwords otherwise.  One launch, asynchronous. */
#define AZMI_WINDOW_MAX_SEGMENTS 64
typedef struct azmi_select_record {
  double threshold_key;
  uint64_t selected;
  uint32_t nan_rows;
  uint32_t first_bad_row;
} azmi_select_record;
int azmi_samples_reservoir_keys(const int32_t* dev_iters, const uint64_t* dev_row_ids, uint32_t n, double iteration, double decay,
                                uint64_t seed, double* dev_keys_out, uint64_t* dev_bits_out, int device, void* stream);
int azmi_samples_select_top(const double* dev_keys, uint32_t n, uint32_t k, int64_t* dev_index_out, azmi_select_record* host_record_out,
                            int device, void* stream);
int azmi_samples_window_gather(const void* const* dev_segments, const uint64_t* segment_rows, uint32_t n_segments, uint32_t row_bytes,
                               const int64_t* dev_index, uint64_t seed, uint64_t pass_index, uint64_t first, uint32_t rows, void* dev_out,
                               int device, void* stream);

/* ---- the participation ratio of a feature matrix (NNWrapper.effective_rank, neural_net.py:865-873; csrc/feature_rank_kernels.h,
 *      DESIGN.md §8.5.3).  The conventions of the blocks above.  dev_features: [n][C] float32, 1 <= C <= 2048.  In float64: the column
 *      means (a first pass), G = Fc^T Fc of the centred columns (a second pass; never S2 - S1 S1^T / n), trace = tr G = the sum of
 *      the squared singular values of Fc, frob2 = |G|_F^2 = the sum of their fourth powers, rank = trace^2 / frob2 - the
 *      reference's figure without an SVD.  frob2 == 0 exactly (one row, equal rows) gives rank 1.0, n == 0 gives NaN and touches no
 *      device.  Every sum runs in an order fixed by (n, C): two calls return the same bits.  dev_mean_out ([C] float64) and
 *      dev_gram_out ([C][C] float64, both triangles) may be NULL.  Five launches; synchronises `stream` once, to hand back the
 *      record; the scratch block is kept per device. */
#define AZMI_FEATURE_RANK_MAX_CHANNELS 2048
typedef struct azmi_feature_rank_record {
  double trace;
  double frob2;
  double rank;
  uint32_t n;
  uint32_t channels;
} azmi_feature_rank_record;
int azmi_samples_feature_rank(const float* dev_features, uint32_t n, uint32_t C, double* dev_mean_out, double* dev_gram_out,
                              azmi_feature_rank_record* host_record_out, int device, void* stream);

/* ---- the stand-alone MCTS class (py_wrapper.cc:192-220, mcts.h:50-200): one search tree driven call by call.
 * All five games.  A GameState argument is passed as start position (`init`, NULL = initial position, else the
 * game's serialized image as in azmi_game_replay_from) + the moves played from it.  The object owns one pcg32
 * stream (the reference shares a thread_local one across all trees of a thread). */
typedef struct azmi_mcts azmi_mcts;
typedef struct azmi_mcts_config {   /* ctor arguments, mcts.h:52-72 */
  float cpuct; uint32_t num_players, num_moves;
  float epsilon, root_policy_temp, fpu_reduction;
  int32_t relative_values, root_fpu_zero, shaped_dirichlet, gumbel_enabled;
  uint32_t gumbel_m; float gumbel_c_visit, gumbel_c_scale; int32_t gumbel_full;
  uint32_t max_simulations;         /* arena size: simulations over the object's lifetime (0 = 50000) */
} azmi_mcts_config;
int azmi_mcts_create(int game, const azmi_mcts_config* cfg, uint64_t seed, int device, azmi_mcts** out);
void azmi_mcts_destroy(azmi_mcts* m);
/* find_leaf(gs): leaf_moves[0 .. *leaf_len) are the moves from gs to the leaf (leaf GameState = gs + those moves) */
int azmi_mcts_find_leaf(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len,
                        int32_t* leaf_moves, uint32_t cap, uint32_t* leaf_len);
/* process_result(gs, value, pi, root_noise_enabled); value_out [P+1] = the reference's in-out `value` afterwards */
int azmi_mcts_process_result(azmi_mcts* m, const float* value, const float* pi, int root_noise_enabled, float* value_out);
/* update_root(gs, move); returns AZMI_ERR_INVALID with "ahh, what is this move" for a move the root does not have */
int azmi_mcts_update_root(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len, uint32_t move);
/* WU-UCT batched search (mcts.h:124-129, mcts.cc:752-851; Python: py_wrapper.cc:212-215).  find_leaf_batched descends with the
 * in-flight penalty (Node::n_in_flight in PUCT's denominator and parent count), appends an entry to the in-flight list and returns
 * the leaf like find_leaf; the entry's index is in_flight_count() - 1.  process_result_batched(leaf_index, ...) backs one entry up
 * (AZMI_ERR_RANGE for an index that is not in the list: the reference's in_flight_.at() -> IndexError); reset_batch() clears the
 * list (at most 1024 entries between resets).  The batched descent is plain PUCT also when Gumbel is enabled, like the reference. */
int azmi_mcts_find_leaf_batched(azmi_mcts* m, const uint8_t* init, uint32_t init_bytes, const int32_t* moves, uint32_t len,
                                int32_t* leaf_moves, uint32_t cap, uint32_t* leaf_len);
int azmi_mcts_process_result_batched(azmi_mcts* m, uint32_t leaf_index, const float* value, const float* pi, int root_noise_enabled,
                                     float* value_out);
int azmi_mcts_in_flight_count(const azmi_mcts* m, uint32_t* out);
int azmi_mcts_reset_batch(azmi_mcts* m);
/* read-outs and small mutations, kind: 0 counts (u32 [M]) 1 probs(temp) 2 probs_pruned(temp) (f32 [M]) 3 root_value (f32 [3])
 * 4 root_q_values (f32 [M]) 5 scalars: u = {depth, root_n, root children}, f = {avg_leaf_depth, normalized_root_entropy}
 * 6 gumbel_improved_policy (f32 [M]) 7 gumbel_final_action (u[0]) 8 add_root_noise 9 apply_root_policy_temp
 * 10 pick_move: in_f = pi [M], u[0] = move 11 principal_variation(depth = arg): u[0] = length, u[1..] = moves
 * 12 set_gumbel_num_sims(arg).  out_f / out_u are HOST arrays of at least max(M, 64) entries (may be NULL if unused). */
int azmi_mcts_query(azmi_mcts* m, uint32_t kind, float temp, uint32_t arg, const float* in_f, float* out_f, uint32_t* out_u);

/* ---- batched position search: `n_trees` independent MCTS trees, each on its own position, advanced together - what the
 * reference's evaluation tools do with a list of MCTS objects stepped in lock step, leaves batched into one net call and one
 * shared S3FIFOCache (frozen_eval.py:545-660, mcts_analysis.py:923-1049, play.py:292-343; moves: further down).  All five games.
 * Tree i is bit for bit the stand-alone azmi_mcts created with seed seeds[i] and driven call by call from the same position
 * with the same evaluator values.  Every tree runs exactly one simulation per step (a terminal leaf or a cache hit is one
 * too, mcts.cc:500-555), so a search of `visits` is `visits` step pairs.
 *   create   cfg as for azmi_mcts_create; cfg->max_simulations sizes EVERY tree's arena and is required (0 is an error; at
 *            most 8000 for the wide games); a size that does not fit the device fails with the byte count in the message
 *   reset    positions + streams, trees emptied: tree i = start position init + i * init_stride (NULL = the initial position;
 *            images as in azmi_game_replay_from, rows zero-padded to one stride) + moves[move_offsets[i] .. move_offsets[i + 1]);
 *            its pcg32 stream is seeded seeds[i] the way azmi_mcts_create seeds its one stream.  HOST arrays.  An illegal move
 *            or a malformed image fails the call with AZMI_ERR_INVALID naming the (first) tree; call reset again to go on
 *   run      `visits` x (find leaves -> leaf net over the compacted row list -> cache insert -> process results), enqueued on
 *            `stream` with no host synchronisation: the row count of a step stays on the device.  net == NULL: every leaf is
 *            evaluated with dumb_eval (EvalType::RANDOM).  cache (or NULL; ignored without a net): an azmi_cache in the
 *            engine's layout (shards = max_size / 64) probed by every leaf and fed with every net answer; a hit takes no row.
 *            Asynchronous: errors of the device side (arena overflow) surface at the next query / sync.  Running past
 *            max_simulations fails with AZMI_ERR_OVERFLOW before anything is enqueued.
 *   find_leaves / process_results   the step API for any evaluator: one simulation's descent of every tree; terminal leaves
 *            are backed up at once, every other leaf's canonical planes become one row of *dev_canonical [*n_rows, C, H, W]
 *            (device memory owned by the object, rows in ascending tree order) with its tree index in *dev_tree_index
 *            [*n_rows]; synchronises `stream` to report *n_rows.  process_results takes the evaluator's answers by row:
 *            dev_v [n_rows, P+1], dev_pi [n_rows, M] probabilities (device memory), asynchronous on `stream`.
 *            leaves_to_host / process_results_host: the same through HOST arrays.
 *   query    the read-outs of azmi_mcts_query for all trees in one launch; kinds 0-7 and 11, and 12 set_gumbel_num_sims(arg)
 *            (run does that itself with arg = visits).  out_f is a HOST array [n_trees, max(M, 64)], out_u
 *            [n_trees, max(M, 64) + 64], row i laid out as azmi_mcts_query lays out its one row (either may be NULL)
 *   sync     waits for everything enqueued and reports a device-side error
 *   stats    out[6] = kernel launches enqueued by the object since creation (the net's own launches not included), net calls,
 *            steps, simulations / leaves given to the evaluator / terminal leaves since the last reset (summed over the trees)
 *   set_leaves_per_step   k in [1, 64] leaves of EVERY tree in flight per step (WU-UCT; 1, the default, is everything above
 *            unchanged).  With k > 1 a step of tree i is k calls of azmi_mcts_find_leaf_batched, each seeing the in-flight marks
 *            of the ones before it; a leaf that needs no evaluator (terminal, dumb_eval, cache hit) gets its
 *            azmi_mcts_process_result_batched at once, the others become rows of ONE evaluator call and are backed up in
 *            ascending order behind it, then reset_batch: play.py:_run_one_batch with the attempt count fixed at k (the
 *            reference goes on "until k misses or 2k attempts", which a lock-step batch cannot budget).  Tree i stays bit for
 *            bit the stand-alone azmi_mcts driven by those calls.  Rows are ordered by tree, then by descent: *dev_tree_index
 *            repeats a tree, and [*n_rows] may reach n_trees * k.  run(visits) is visits / k steps and one of visits % k
 *            descents; max_simulations and `simulations` count descents, `steps` counts steps; a find_leaves with fewer than k
 *            descents left runs those.  Two in-flight leaves on one position both miss the cache and are both evaluated.
 *            Legal before the first reset and after a reset, before anything is searched; (re)allocates the in-flight records
 *            and step-sized row buffers and fails with the byte count when they do not fit.  gumbel_enabled with k > 1 is
 *            AZMI_ERR_INVALID: the batched descent is plain PUCT (mcts.cc:752-784)
 *   set_descents_per_step   l in [1, 256] descents of a tree per step of run / play (1, the default, is everything above
 *            unchanged: the same launches with the same arguments, nothing read back).  With l > 1 a step of a live tree is the
 *            per-tree loop of mcts_analysis.py:921-951: up to l x { find_leaf; a terminal leaf, a dumb_eval leaf (RANDOM) or a
 *            cache hit gets its process_result at once and the loop goes on; the first leaf that needs the net (PLAYOUT: a
 *            rollout) becomes the tree's ONE row of the step and ends it }, then one evaluator call, the cache insert and the
 *            back-up of the pending rows as with l == 1.  Tree i makes the same find_leaf / process_result calls in the same order
 *            as with l == 1 and stays bit for bit the stand-alone azmi_mcts; only the cache's hit / miss counts and eviction state
 *            may differ.  The j-th rollout of a tree keeps its seed.  Gumbel batches are supported (the K == 1 descent).
 *            run(visits) / every move of play gives every live tree exactly `visits` descents through a per-tree device counter
 *            set by one launch: RANDOM enqueues exactly ceil(visits / l) steps and reads nothing; with a net or PLAYOUT the call
 *            enqueues ceil(visits / l) steps, then repeats { read r = the largest count left (ONE 4-byte word, synchronising
 *            `stream`); stop at 0; enqueue m more steps }, m = ceil(r / l) behind the first read (the fewest that can finish),
 *            max(ceil(r / l), twice the previous m) behind every later one, never more than r.  Every step gives every tree that
 *            owes descents at least one: at most 1 + ceil(log2(visits)) reads, counted by host_reads.  `steps` of stats counts enqueued steps, those with no work left included.  play picks a move only behind
 *            the read of 0.  Same state rules as set_leaves_per_step.  AZMI_ERR_INVALID before any launch: l > 1 together with
 *            leaves_per_step > 1 (from either setter), run_to and find_leaves on a batch with l > 1 (the checkpoint launches are
 *            planned for one descent per step; the step API's caller owns the step).
 *   host_reads   *out = the 4-byte reads run / play have made for descents_per_step > 1 since creation */
typedef struct azmi_search azmi_search;
int azmi_search_create(int game, const azmi_mcts_config* cfg, uint32_t n_trees, int device, azmi_search** out);
void azmi_search_destroy(azmi_search* s);
int azmi_search_reset(azmi_search* s, const uint8_t* init, uint32_t init_stride, const int32_t* moves, const uint32_t* move_offsets,
                      const uint64_t* seeds);
int azmi_search_find_leaves(azmi_search* s, void* stream, float** dev_canonical, uint32_t** dev_tree_index, uint32_t* n_rows);
int azmi_search_process_results(azmi_search* s, const float* dev_v, const float* dev_pi, int root_noise_enabled, void* stream);
int azmi_search_leaves_to_host(azmi_search* s, float* canonical, uint32_t* tree_index);
/* the engine key (hash_game_state, game_state.h:141-156; cache_utils.py:24) of every row of the pending find_leaves step, in row
 * order: *dev_keys = [*n_rows] uint64 in a buffer of the object, valid until the next find_leaves.  The find kernel hashed every
 * leaf it handed out (the hash search and capture_roots use); one launch brings the keys into row order, then `stream` is
 * synchronised, since the caller's evaluator runs on a stream of its own.  With leaves_per_step > 1 the keys are the ones a search
 * with a cache would insert under: a key of 0 reads 0x9E3779B97F4A7C15, the value every cache stores it as.  AZMI_ERR_STATE when no
 * step is pending. */
int azmi_search_leaf_keys(azmi_search* s, void* stream, uint64_t** dev_keys, uint32_t* n_rows);
int azmi_search_process_results_host(azmi_search* s, const float* v, const float* pi, int root_noise_enabled);
typedef struct azmi_net azmi_net;
int azmi_search_run(azmi_search* s, azmi_net* net, azmi_cache* cache, uint32_t visits, int root_noise_enabled, void* stream);
int azmi_search_query(azmi_search* s, uint32_t kind, float temp, uint32_t arg, float* out_f, uint32_t* out_u);
int azmi_search_sync(azmi_search* s);
int azmi_search_stats(azmi_search* s, uint64_t out[6]);
int azmi_search_set_leaves_per_step(azmi_search* s, uint32_t k);
int azmi_search_set_descents_per_step(azmi_search* s, uint32_t l);
int azmi_search_host_reads(azmi_search* s, uint64_t* out);
/* ---- moves on a batched search: what the evaluation tools do between two searches of a game they walk (play.py:274-346,
 * mcts_analysis.py:995-1051): pick a move, MCTS::update_root on every tree (mcts.cc:151-173), search the successor with the reused
 * subtree.  The root state of every tree is advanced on the device; tree i stays bit for bit the stand-alone azmi_mcts driven by
 * the same calls.  A tree whose game is over (a played move reached a terminal state) is FINISHED: every step skips it, its
 * read-outs stay legal, it takes no further move.  A pending find_leaves step makes the four calls below that change the trees
 * fail with AZMI_ERR_STATE; game_state is a read-out and stays legal.  A NULL handle is what a caller holds whose create
 * failed: the five calls answer it with AZMI_ERR_NO_DEVICE on a machine without a HIP device (the reason create failed there) and
 * with AZMI_ERR_INVALID on one with a device.
 *   pick_moves    m.pick_move(m.probs(temp)) of every live tree, drawn from the tree's own stream (MCTS::probs mcts.cc:575-618,
 *                 MCTS::pick_move mcts.cc:717-735); a Gumbel tree takes gumbel_final_action() (mcts.cc:375-401), no draw.  The
 *                 moves stay on the device for update_roots(NULL); host_moves [n_trees] (may be NULL: nothing is read back,
 *                 the call is asynchronous) receives them, -1 for a finished or stopped tree.  A root without visits takes no
 *                 move: AZMI_ERR_STATE naming the tree at the next synchronising call; the tree is left as it was.
 *   update_roots  MCTS::update_root(gs, move) (mcts.cc:151-173: an unexpanded root is expanded first; the Gumbel state is
 *                 reset) + gs.play_move(move) on every live tree i with moves[i] >= 0, the move appended to the tree's log; a
 *                 terminal successor finishes the tree.  host_moves NULL: the moves of the last pick_moves, asynchronous; a
 *                 pick is played once (reset and update_roots leave "no move" behind, so without a new pick nothing moves).
 *                 HOST array otherwise, and the call synchronises: a move the root does not have ("ahh, what is this move",
 *                 mcts.cc:163) fails with AZMI_ERR_INVALID naming the tree; THAT tree is left where it was and stays live, the
 *                 other trees' moves of the call are applied.  The wide games compact their arenas behind it (the PlayManager
 *                 engine's k_compact: the live subtree moves to the idle half when the active one is filling up).
 *   root_prior    MCTS::apply_root_policy_temp (mcts.cc:448-460) when apply_temp, then MCTS::add_root_noise (mcts.cc:403-446)
 *                 when add_noise, on the root of every live tree: what PlayManager does to a reused root
 *                 (play_manager.cc:523-555).  Asynchronous.
 *   play          max_moves x { the steps of run(visits, root_noise), pick_moves(temp), update_roots(NULL), root_prior(root
 *                 temperature != 1, root_noise) when either holds }: play.py:274-346's loop, enqueued on `stream` with nothing
 *                 read back.  A move adds 2 launches to its search steps (3 for the wide games: the compaction; one more with
 *                 the root prior), whatever n_trees is.
 *   game_state    synchronises; HOST arrays, any may be NULL: status [n_trees] (0 live, 1 finished), log_len [n_trees], log
 *                 [n_trees, cap] with cap = the game's max_turns + 8 (the moves played since reset; Connect4 42, Brandubh 150,
 *                 Tawlbwrdd / OpenTafl 400, StarGambit 4096 turns), final_scores [n_trees, P+1] (GameState::scores() of a
 *                 finished tree; rows of live trees are unspecified)
 * The simulation budget.  max_simulations sizes the arena, and the two arena kinds differ.  Connect4's flat arena never reclaims:
 * the budget counts every descent since reset(), the searches of all moves included (a game needs visits x moves).  The wide
 * games' arenas have two halves and update_roots compacts them, reclaiming the discarded siblings (the PlayManager engine's
 * rule): the budget counts the descents since the last update_roots that gave every tree a move and saw none refused.  run, find_leaves and play check it
 * before they enqueue anything (AZMI_ERR_OVERFLOW; the message names the rule); `simulations` of stats counts everything since
 * reset. */
int azmi_search_pick_moves(azmi_search* s, float temp, int32_t* host_moves, void* stream);
int azmi_search_update_roots(azmi_search* s, const int32_t* host_moves, void* stream);
int azmi_search_root_prior(azmi_search* s, int apply_temp, int add_noise, void* stream);
int azmi_search_play(azmi_search* s, azmi_net* net, azmi_cache* cache, uint32_t visits, float temp, uint32_t max_moves, int root_noise,
                     void* stream);
int azmi_search_game_state(azmi_search* s, int32_t* status, uint32_t* log_len, int32_t* log, float* final_scores);
/* ---- the evaluator of a batched search named outright, EvalType::PLAYOUT among them (play.py:306, mcts_analysis.py:649,
 * game_state.cc:10-95).  run_eval / play_eval are run / play with eval_type (azmi_eval_type): AZMI_EVAL_NN needs a net,
 * AZMI_EVAL_RANDOM and AZMI_EVAL_PLAYOUT take none, AZMI_EVAL_PLAYOUT takes no cache either (the reference's playout branch sits
 * before its cache probe); anything else is AZMI_ERR_INVALID before a launch.  run / play are these with NN when a net is given and
 * RANDOM otherwise.  The step API (find_leaves / process_results) is the same for every evaluator.
 *   AZMI_EVAL_PLAYOUT   every non-terminal leaf is evaluated as azmi_playout_eval evaluates it - the uniform policy over its legal
 *                 moves (u8 sum wrap of dumb_eval), the scores of one uniformly random rollout, 1 / (P + 1) each if the rollout
 *                 cannot reach an end - on the device, and backed up by the unchanged process_result.  Every rollout has a FRESH
 *                 pcg32 stream, so a tree's result does not depend on n_trees, on leaves_per_step's launch shape or on the other
 *                 trees: the j-th rollout of tree i since reset (j from 0, in descent order, running on across moves) is seeded
 *                 mix64(rollout_seeds[i] + 0x9E3779B97F4A7C15 * (j + 1)) the way azmi_playout_eval seeds its stream from seeds[g],
 *                 with mix64 the splitmix64 finaliser of x + 0x9E3779B97F4A7C15.  With leaves_per_step > 1 a playout leaf is an
 *                 immediate: its process_result_batched runs at once, in descent order, before the tree's next descent
 *                 (play.py:306-307).  No compaction, no net call, no cache insert: a step is at most 3 launches whatever
 *                 n_trees and leaves_per_step are.  `leaves given to the evaluator` of stats counts the rollouts.
 *   set_rollout_seeds   rollout_seeds[i] of every tree from a HOST array [n_trees]; NULL: the default, which every reset
 *                 restores, mix64(seeds[i] ^ 0x9E3779B97F4A7C15) of the reset's seeds.  After a reset; the rollout counts are
 *                 the reset's to clear.  Synchronises. */
int azmi_search_run_eval(azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, uint32_t visits, int root_noise_enabled, void* stream);
int azmi_search_play_eval(azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, uint32_t visits, float temp, uint32_t max_moves,
                          int root_noise, void* stream);
int azmi_search_set_rollout_seeds(azmi_search* s, const uint64_t* seeds);
/* ---- search to per-tree visit targets, snapshots at checkpoints: the inner loop of mcts_analysis.py:run_analysis
 * (mcts_analysis.py:884-972, batched :975-1063) - `while mcts.root_n() < target: find_leaf / evaluate / process_result`, with
 * probs(temp) | probs_pruned(temp) and root_value() captured once at every smaller visit count of the sweep (:903-905, :960-972).
 *   run_to        tree i descends while root_n(i) < targets[i] (HOST array [n_trees]); a tree at or above its target, a finished
 *                 or a stopped tree takes no descent.  A reused root (update_roots) already holds visits, so it needs fewer
 *                 descents than its target.  `checkpoints`: HOST array of n_checkpoints <= 32 strictly ascending positive visit
 *                 counts, or NULL with 0.  Snapshot j of tree i is taken once, on the device, at the first step boundary at which
 *                 root_n(i) >= checkpoints[j] - before the first descent for a tree that starts there; a checkpoint above the
 *                 tree's target is never taken.  With leaves_per_step = K > 1 every step is K descents of every tree still below
 *                 its target (a tree may overshoot by fewer than K, mcts_analysis.py:982-1058) and the snapshots are taken at
 *                 step boundaries.  Evaluator, net, cache and root noise are run_eval's.  The call reads root_n of every tree once
 *                 (it synchronises `stream` for that), then enqueues T = max_i ceil((targets[i] - root_n(i)) / K) steps and reads
 *                 nothing back; the budget (see above) is checked for T * K descents before anything is enqueued.  The
 *                 checkpoint kernel runs only at the steps at which, by root_n(i) + t * K, some tree newly reaches a checkpoint or
 *                 its target, and once behind the last step: `launches` of stats rises by those of run_eval(T * K) plus the
 *                 number of such steps, whatever n_trees is (the read before the run is not counted).  A tree at its target is
 *                 held out of the remaining steps by a status of its own that the call's last launch clears on every return
 *                 path, so that game_state never shows it.  Every call starts a fresh snapshot set.  A Gumbel batch is
 *                 AZMI_ERR_INVALID: sequential halving plans a fixed budget at its first descent, and a root_n target on a reused
 *                 tree is not one.
 *   checkpoints   the snapshot set of the last run_to into HOST buffers, any of them NULL: taken_mask [n_trees] (bit j: snapshot j
 *                 was taken), root_n [n_trees, J], counts [n_trees, J, M], probs [n_trees, J, M] (probs(temp), or
 *                 probs_pruned(temp) with `pruned`), root_values [n_trees, J, 3], root_q [n_trees, J, M]; rows not taken are zero.
 *                 Synchronises.  AZMI_ERR_STATE before any run_to. */
int azmi_search_run_to(azmi_search* s, int eval_type, azmi_net* net, azmi_cache* cache, const uint32_t* targets, const uint32_t* checkpoints,
                       uint32_t n_checkpoints, float temp, int pruned, int root_noise_enabled, void* stream);
int azmi_search_checkpoints(azmi_search* s, uint32_t* taken_mask, uint32_t* root_n, uint32_t* counts, float* probs, float* root_values,
                            float* root_q);
/* ---- scoring a visit sweep against its anchor: the second half of mcts_analysis.py:run_analysis (:1150-1400), on the snapshot
 *      set run_to left on the device (csrc/search_sweep_metrics_kernels.h).  Everything in float64, the float32 snapshot values
 *      converted exactly; the reference computes in float32 numpy, which nothing can be matched bit for bit against.
 *   sweep_metrics  `ref`: another azmi_search of the same game, tree count and device, or NULL for `s` itself; its snapshot set
 *                 supplies the anchor row, the raw row and root_q (the reference's `base_ref` tree when the swept trees are
 *                 self-play-mode ones).  `anchor`, `raw`: checkpoint indices into ref's set, raw = -1 for none.  `outcomes`: HOST
 *                 array [n_trees] of game outcomes, or NULL.  With p = ref.probs[i, anchor], r = ref.probs[i, raw], Q =
 *                 ref.root_q[i, anchor], v = root_values[..., 0] and row (i, j): q = probs[i, j], the 15 columns of out_rows are,
 *                 policy_metrics.py and mcts_analysis.py:1196-1258 expression for expression,
 *                   0 jsd        0.5 sum_{p>0} p ln(p / m) + 0.5 sum_{q>0} q ln(q / m), m = 0.5 (p + q)
 *                   1 tv         0.5 sum |p - q|
 *                   2 hellinger  sqrt(0.5 sum (sqrt p - sqrt q)^2)
 *                   3 top1, 4 top3, 5 top9   |top_k(p) & top_k(q)| / k.  top_k(x) = the last k indices of x ordered ascending by
 *                                (value, index), np.argsort(x, kind="stable")[-k:]: among equal values the higher index ranks
 *                                higher.  This rule is the project's definition (the reference's default argsort is not stable
 *                                for every M and numpy build).  With M < k every index is in both sets and the divisor stays k.
 *                   6 reward     sum q Q            7 regret   reward of the anchor row - reward
 *                   8 pressure   sum_{q>0} q ln(q / (r + 1e-10))        9 benefit  reward - sum r Q
 *                  10 entropy    -sum_{q>0} q ln q                     11 value_gap  |v_j - v_anchor|
 *                  12 abs_err    |v_j - outcome|   13 closer_than_anchor  1.0 if |v_j - o| < |v_anchor - o| else 0.0
 *                  14 closer_than_raw  1.0 if |v_j - o| < |v_raw - o| else 0.0
 *                 and out_tree[i] = the ceiling KL(p || r + 1e-10).  Row (i, j) is valid when snapshot j of tree i and ref's
 *                 anchor snapshot of tree i were both taken; an invalid row is NaN in every column.  Columns 8, 9, 14 and
 *                 out_tree are NaN when raw is -1 or ref's raw snapshot of the tree was not taken; columns 12-14 are NaN without
 *                 outcomes.  out_mean[j, c] / out_count[j, c]: the mean over, and the number of, the trees whose row (i, j) is
 *                 not NaN in column c (NaN for a count of 0), summed in a fixed order: the bits do not depend on scheduling.
 *                 Two launches (rows, means) whatever n_trees and J are, and one synchronisation (a `ref` or a snapshot set last
 *                 used on another stream is waited for first).  HOST buffers, any of them NULL: out_rows [n_trees, J, 15] f64,
 *                 out_tree [n_trees] f64, out_mean [J, 15] f64, out_count [J, 15] u32, valid [n_trees, J] u8.  The output block is
 *                 allocated by the first call; no tree and no snapshot is changed.  AZMI_ERR_STATE before any run_to on s or ref,
 *                 or while a find_leaves step is pending; AZMI_ERR_INVALID for an index out of range or a ref of another game,
 *                 tree count or device; the object stays usable.
 * azmi_policy_divergences is columns 0-5 as one call on HOST float32 arrays p, q [rows, M] -> out [rows, 6] f64, by the same row
 * function (the batch_* functions of policy_metrics.py, per row).  rows == 0 is legal and touches no device; M == 0, M > 2^20 or
 * rows > 2^30 is AZMI_ERR_INVALID.  `stream`: a HIP stream or NULL; the call synchronises it. */
int azmi_search_sweep_metrics(azmi_search* s, azmi_search* ref, uint32_t anchor, int32_t raw, const double* outcomes, double* out_rows,
                              double* out_tree, double* out_mean, uint32_t* out_count, uint8_t* valid, void* stream);
int azmi_policy_divergences(const float* p, const float* q, uint32_t rows, uint32_t M, double* out, int device, void* stream);
/* ---- a frozen evaluation set on the device: the two parts of frozen_eval.py around its search loop.  _burst_capture_one_variant
 * (frozen_eval.py:330-413) plays whole games and keeps every position it has not seen yet; the metric extraction
 * (frozen_eval.py:573-575, 649-672) compares every searched root with one raw forward of the net.
 *   set_capture   on != 0: every play_eval move records the root of every live tree (status == 0) BEFORE that move's search, one
 *                 launch per move: at [tree][ply], ply = the tree's move-log length, the engine key of the root state (what
 *                 azmi_game_replay returns as `key`), the player to move and the variant (-1 except StarGambit).  Capturing a ply
 *                 twice stores the same values.  The arrays ([n_trees, max_turns + 8] each) are allocated by the first call that
 *                 turns capture on; with capture off nothing is allocated or launched.  reset clears the captured lengths.
 *   capture_roots the same launch for a caller that walks run / pick_moves / update_roots itself.  AZMI_ERR_STATE with capture off.
 *   captured      the records into HOST buffers, any of them NULL: key / player / variant [n_trees, max_turns + 8], len [n_trees]
 *                 (entries at ply >= len[tree] are unspecified).  Synchronises.  AZMI_ERR_STATE if capture was never on.
 *   net_metrics   for every tree that is live and whose root is not terminal: the net's raw (v, pi) of the root's canonical planes
 *                 and, in float64, out[tree] = { KL(counts / total || raw_pi + 1e-10), mean |raw_v - root_value|, 1.0 if the
 *                 arg-maxes of counts and raw_pi agree (first index wins) } - counts / total is uniform 1 / M for a root without
 *                 visits.  Three launches (root planes, the net over all n_trees rows, the comparison) and one synchronisation.
 *                 HOST buffers, any of them NULL: out [n_trees, 3] f64, raw_v [n_trees, P + 1], raw_pi [n_trees, M], valid
 *                 [n_trees] u8.  A tree that takes no part has valid = 0 and NaN in every row.  AZMI_ERR_STATE while a find_leaves
 *                 step is pending.
 * azmi_pool_unique is the `seen_keys` set of the capture loop as one call on HOST arrays: of the n records with valid[i] != 0
 * (valid NULL = all), first_index_out[0 .. *n_unique) are, ascending, the indices i for which no valid j < i has keys[j] ==
 * keys[i]; *n_duplicates = the valid records left out.  Every 64-bit value is a key, 0 included.  The result does not depend on
 * scheduling.  n == 0 is legal and touches no device; n > 2^30 is AZMI_ERR_INVALID (the table of at least 2 n slots is indexed
 * by 32 bits).  `stream`: a HIP stream or NULL; the call synchronises it. */
int azmi_search_set_capture(azmi_search* s, int on);
int azmi_search_capture_roots(azmi_search* s, void* stream);
int azmi_search_captured(azmi_search* s, uint64_t* key, uint8_t* player, int8_t* variant, uint32_t* len);
int azmi_search_net_metrics(azmi_search* s, azmi_net* net, double* out, float* raw_v, float* raw_pi, uint8_t* valid, void* stream);
int azmi_pool_unique(const uint64_t* keys, const uint8_t* valid, uint32_t n, uint32_t* first_index_out, uint32_t* n_unique,
                     uint32_t* n_duplicates, int device, void* stream);

/* ---- opening trees by reach probability (the reference's opening_analysis.py build_tree, :261-355): the step from n_trees
 *      searched roots to the next level's frontier, on the device (csrc/search_frontier_kernels.h).  Everything in float64.
 *   expand    `reach`, `temp`: HOST arrays [n_trees], the reach probability and the sampling temperature of every tree.  Per
 *             tree: kind = 0 a searched live root, 1 a terminal root (value = its scores(), no policies, no children), 2 the
 *             tree takes no part (finished, stopped, or reach == 0: zero rows).  For kind 0, expression for expression:
 *             raw_pi = counts / total (evaluate_node, :233-257), uniform over the root's legal moves when total == 0, on a
 *             Gumbel batch the improved policy over its float64 sum when that sum is positive; sampling_pi = apply_temperature
 *             (play.py:256-266): one-hot at the first arg-max for temp == 0, raw_pi for temp == 1, else (raw_pi + 1e-10) **
 *             (1 / temp) over its sum; entropy = -sum over p > 0 of p ln p; value = root_value(); key = the root's engine key.
 *             Move a is kept when sampling_pi[a] > 0 and reach * sampling_pi[a] >= min_reach and a is legal at the root (the
 *             reference would raise from play_move where the `+ 1e-10` gives an illegal move its tiny mass).  Every kept move
 *             becomes one record, in (tree, action) order: parent, action, child_reach = reach * sampling_pi[a] and, from the
 *             root state with the action played on a copy, the successor's engine key, player to move, variant (-1 except
 *             StarGambit), terminal flag and scores() [P + 1] (zeros unless terminal).  A record at or beyond `max_children`
 *             is not written; the total is still exact.  Exactly three launches, whatever n_trees is (policies, a scan of the
 *             kept counts, records); asynchronous.  The buffers are allocated by the first call and regrown when max_children
 *             grows; with no call nothing is allocated or launched.  No tree is changed.  min_reach <= 0, a negative or
 *             non-finite reach or temp, or max_children == 0: AZMI_ERR_INVALID before any launch; AZMI_ERR_STATE while a
 *             find_leaves step is pending.
 *   frontier  the result of the last expand into HOST buffers, any of them NULL; synchronises once.  Per tree: kind [n_trees]
 *             u8, key [n_trees], raw_pi / sampling_pi [n_trees, M] f64, entropy [n_trees], value [n_trees, 3], first_child
 *             [n_trees + 1] (the records of tree i are first_child[i] .. first_child[i + 1]; first_child[n_trees] = the total).
 *             Per record, `total` entries each (buffers with room for the expand's max_children always do): parent, action,
 *             child_reach, child_key, child_player, child_variant, child_terminal, child_scores [total, P + 1].  A total above
 *             max_children is AZMI_ERR_OVERFLOW with a message naming the total and the capacity; the per-tree buffers are
 *             filled, the batch stays usable, and an expand with room gives the full answer.  AZMI_ERR_STATE before any expand.
 *      A NULL handle is AZMI_ERR_NO_DEVICE without a device, AZMI_ERR_INVALID with one, as for the move entry points. */
int azmi_search_expand(azmi_search* s, const double* reach, const double* temp, double min_reach, uint32_t max_children, void* stream);
int azmi_search_frontier(azmi_search* s, uint8_t* kind, uint64_t* key, double* raw_pi, double* sampling_pi, double* entropy, double* value,
                         uint32_t* first_child, uint32_t* parent, uint32_t* action, double* child_reach, uint64_t* child_key,
                         uint8_t* child_player, int8_t* child_variant, uint8_t* child_terminal, float* child_scores);

/* ---- leaf policy/value network (the reference's NNArch forward + NNWrapper.process,
 *      neural_net.py:448-510, 800-823) as one fused MFMA kernel; ResNet trunks through azmi_net_create, the reference's
 *      default DenseNet trunk (with 1x1 / 5x5 / 7x7 convolutions on the fp32 path) through azmi_net_create2 ----------
 * `blob` is the BatchNorm-folded, MFMA-fragment-ordered weight image produced by
 * alphazero/hip_net.py::fold() (layout documented there and in DESIGN.md); it is copied to HBM.
 * forward(): canonical [batch,C,H,W] f32 -> v [batch,P+1], pi [batch,M] f32 probabilities, all
 * device pointers, asynchronous on `stream`. */
typedef struct azmi_net_desc {
  int32_t in_channels, height, width;   /* CANONICAL_SHAPE */
  int32_t channels, depth, kernel_size; /* NNArgs.num_channels / depth / kernel_size */
  int32_t head_channels, v_hidden;      /* NNArgs.head_channels / v_fc_hidden */
  int32_t num_moves, num_players;
  /* head options (neural_net.py:56-75, 341-427). policy_channels > 0 selects the spatial policy head
   * (POLICY_SHAPE[0]; Tafl family 22, Brandubh 14) and its kernel; 0 = flat FC policy head.
   * bf16 kernels instantiated: 6x7 flat head (64 trunk / 32 head channels), 11x11 and 7x7 spatial head (64 / 64 channels;
   * narrower nets are passed zero-padded to 64 by fold()).  Any other shape: AZMI_ERR_INVALID, or precision = 1. */
  int32_t v_head_convs, pi_head_convs, v_fc_layers, policy_channels;
  /* 0 = bf16 operands on the matrix cores, fp32 accumulation (what the reference runs under autocast,
   * neural_net.py:811-813) — the throughput path.  1 = plain fp32 arithmetic, layer by layer: the precision
   * the 1e-5 parity tier refers to, for any net shape; blob layout in csrc/leafnet_f32.hip.  2 = "bf16x3" (6x7 flat-head
   * family only): the bf16 tile with weights and activations split into bf16 high + low parts, three MFMAs per product -
   * within 1e-5 of the fp32 outputs (measured 4e-7 / 5e-6) at a third of the bf16 rate; blob: the bf16 layout with the
   * stem's fragments twice (high, low) and three chunks [W_hi][W_hi][W_lo] per tap and for the head 1x1 (hip_net.fold). */
  int32_t precision;
  /* spatial head with GLOBAL actions (num_moves > policy_channels * H * W: StarGambit's 18 deploys + end turn,
   * neural_net.py:413-426, 486-493): hidden width of pi_global (NNArgs.pi_fc_hidden); the global logits come from the
   * average-pooled policy features through Linear - ReLU - Linear - LayerNorm and join the softmax behind the spatial block.
   * 0 when the net has no global actions.  bf16 kernel: also instantiated for 13x13 (configs/star_gambit_unified.yaml). */
  int32_t pi_hidden;
} azmi_net_desc;
typedef struct azmi_net azmi_net;
size_t azmi_net_blob_bytes(const azmi_net_desc* desc);
int azmi_net_create(const azmi_net_desc* desc, const void* blob, size_t blob_bytes, int device, azmi_net** out);
/* The second descriptor: azmi_net_desc is full and its layout is ABI, so what came later stands behind it.  The entry points
 * yield the same handle type; dense_net = 0 forwards to azmi_net_blob_bytes / azmi_net_create, which refuse what they refused.
 *   dense_net = 1   the reference's DenseNet trunk (NNArgs.dense_net, the TrainConfig default; neural_net.py:211-230, 302-338): no
 *                   stem, block i = BN - ReLU - 1x1 to 4 * channels - BN - ReLU - k x k to `channels` (the growth rate) -
 *                   concatenation; the heads read in_channels + channels * depth features.
 *                   precision 0: one matrix-core kernel for the dense Connect4 family (csrc/leafnet_dense.h) - 6x7, flat policy
 *                   head, kernel_size 3 or 5, 1 <= channels <= 16, depth >= 1, in_channels + channels * depth <= 128,
 *                   head_channels 32, no extra head convolutions, v_fc_layers 1, v_hidden a multiple of 16 up to 256,
 *                   num_players <= 3, num_moves <= 16; narrower widths are zero-padded by fold().  And a second one for the dense
 *                   spatial-head family (csrc/leafnet_dense_sp.h: the single-variant StarGambit configs) - policy_channels 1..32 on
 *                   7x7, 11x11 or 13x13, 0..32 global actions (pi_hidden a multiple of 16 in 16..256 with them), the same trunk
 *                   and value-head bounds, trunk_norm 0 only.  Everything else, and precision 2, is AZMI_ERR_INVALID with a
 *                   message naming precision='fp32'.
 *                   precision 1: any dense shape (every head the fp32 path has), kernel_size 1, 3, 5 or 7 for the trunk and the
 *                   extra head convolutions.
 *   trunk_norm      0 = nn.BatchNorm2d on every trunk norm (folded on the host), 1 = "layer": nn.GroupNorm(1, C) (NNArgs.trunk_norm,
 *                   neural_net.py:166-180) - mean and biased variance per sample over (C, H, W), eps 1e-5, then a per-channel weight
 *                   and bias; the ResNet stem's norm and bn1 / bn2 of every block.  The heads keep their folded BatchNorms.
 *   trunk_act       0 = ReLU, 1 = "crelu": cat(relu(x), relu(-x)) (NNArgs.trunk_act, neural_net.py:183-208) in front of both
 *                   convolutions of every block, whose weights then have twice the input channels.
 *   pi_fc_layers    L >= 0 (NNArgs.pi_fc_layers, neural_net.py:431-442; flat policy head only: policy_channels must be 0): L > 0
 *                   puts Linear(HC*H*W, pi_hidden) - ReLU - (L-1) x (Linear(pi_hidden, pi_hidden) - ReLU) -
 *                   Linear(pi_hidden, num_moves) in place of the single projection; base.pi_hidden carries its width.
 *                   With any of these three set, dense_net = 0 does NOT forward to azmi_net_create: the second entry handles the
 *                   ResNet trunk itself.  They run on precision 1 (every combination, both trunks, all policy heads; image in
 *                   csrc/leafnet_f32.hip).  On the matrix cores: dense_net = 1, precision 0, trunk_norm = 1 with trunk_act = 0 and
 *                   pi_fc_layers = 0 is the layer-norm instance of the dense Connect4 tile (csrc/leafnet_dense.h; the batch
 *                   instance's bounds; per-board statistics by wave-local reductions).  Everything else on precision 0 / 2 is
 *                   AZMI_ERR_INVALID with a message naming precision='fp32': the ResNet tiles are built around folded BatchNorms,
 *                   the dense tile's LDS plan has no room for crelu's doubled K, and pi_fc_layers > 0 is REFUSED on every tile (the
 *                   dense tile was not given the fp32 stack behind its heads).  A value out of range is AZMI_ERR_INVALID.
 *                   All three zero: both entries behave exactly as before these words had names.
 *   reserved        must be zero (AZMI_ERR_INVALID otherwise; blob_bytes2 returns 0).
 * A dense net runs everywhere an azmi_net does except the asynchronous pipeline, which hard-wires the Connect4 ResNet tile:
 * azmi_pipeline_supported(_groups) return 0 with it and azmi_run_pipeline(_groups) refuse it. */
typedef struct azmi_net_desc2 { azmi_net_desc base; int32_t dense_net; int32_t trunk_norm, trunk_act, pi_fc_layers; int32_t reserved[4]; } azmi_net_desc2;
size_t azmi_net_blob_bytes2(const azmi_net_desc2* desc);
int azmi_net_create2(const azmi_net_desc2* desc, const void* blob, size_t blob_bytes, int device, azmi_net** out);
void azmi_net_destroy(azmi_net* net);
int azmi_net_forward(azmi_net* net, const float* dev_canonical, float* dev_v, float* dev_pi, uint32_t batch, void* stream);
/* the same on a subset of the rows: dev_rows[0 .. *dev_row_count) (device memory, read when the kernel runs) are
 * the row indices to evaluate; rows not listed are left untouched.  The engine lists the slots whose pending
 * leaf really needs the net (cache hits, terminal leaves and retired slots do not). */
int azmi_net_forward_rows(azmi_net* net, const float* dev_canonical, float* dev_v, float* dev_pi, const uint32_t* dev_rows,
                          const uint32_t* dev_row_count, uint32_t max_rows, void* stream);
/* The trunk read-out behind NNWrapper.effective_rank (neural_net.py:826-873: a forward hook on nnet.conv_layers, then
 * feats.mean(dim=(2, 3))), on the fp32 tier, whose forward keeps the trunk's output [batch][CF][H*W] in a buffer of its own.
 *   trunk_channels  *cf = CF: `channels` for a ResNet trunk, in_channels + channels * depth for a dense one (whose features
 *                   begin with the input planes).
 *   trunk_features  the stem and trunk launches of azmi_net_forward and nothing of the heads, then dev_features[b][c]
 *                   (float32 [batch][CF]) = the mean of channel c over the H*W cells, added in ascending cell order by one thread:
 *                   a row's bits do not depend on `batch` or on the row's place in it.  Stream-ordered, no synchronisation with
 *                   the host (it shares the fp32 tier's activation buffers with azmi_net_forward: a call on another stream first
 *                   waits for the previous one, as there).  batch == 0 touches no device.
 * A net of another precision tier (the matrix-core tiles keep their trunk in LDS) fails both with AZMI_ERR_INVALID and a message
 * naming precision='fp32', before any launch. */
int azmi_net_trunk_channels(azmi_net* net, uint32_t* cf);
int azmi_net_trunk_features(azmi_net* net, const float* dev_canonical, float* dev_features, uint32_t batch, void* stream);
/* The hand-off from training back to self-play without the host (the reference reloads a checkpoint once per iteration,
 * game_runner.py:2043-2051): the weight image of a LIVE net rewritten in place from the trained model's float32 parameters where
 * they are in device memory.  Kernels fold the BatchNorms in float64 (a = w / sqrt(var + eps), b = bias - mean * a), lay out the MFMA
 * fragments (double -> float32 -> bf16, both to nearest even; bf16x3: high and low parts) and write the image into a staging copy
 * allocated by the first call; one device-to-device copy on `stream` moves it into the live image.  The result is byte for byte the
 * blob alphazero/hip_net.py::fold() makes of the same parameters.  The handle, its device pointers (azmi_net_c4_view) and every
 * engine holding them stay valid.
 *   params       HOST array, one record per tensor the family's fold reads, in the family's order (alphazero/hip_net.py
 *                refresh_names): `data` = device pointer to contiguous float32 on the net's device, `count` = elements, `kind` as
 *                below, `eps` = the BatchNorm's eps on its running_var record (0 elsewhere), `reserved` = 0.  The count, every kind,
 *                every element count and every pointer's device are checked BEFORE anything is enqueued: a mismatch is
 *                AZMI_ERR_INVALID with a message naming the tensor, and the weights are untouched.
 *   stream       the order: a forward enqueued on `stream` before the call reads the old weights whole, one enqueued after it the new
 *                ones whole.  No host synchronisation (the table goes up as one small pinned copy on the stream) - except that a
 *                call first waits for the previous refresh OF THE SAME NET to finish, whose table and staging image it reuses.  A
 *                forward on ANOTHER stream is the caller's to order against the refresh (an event), as for any write to shared memory.
 * Built for the two Connect4 families self-play runs: the ResNet flat-head tile (precision 0 and 2) and the dense Connect4 tile's
 * batch-norm instance.  Every other family - the spatial-head tiles, the dense spatial tile, the dense layer-norm instance, the fp32
 * tier - answers AZMI_ERR_INVALID "refresh is not built for this family" before any launch: create a new net for those.  A position
 * cache filled under the old weights still serves the old answers: the caller starts a new one (the reference builds one per
 * self_play call, game_runner.py:2013-2060). */
enum { AZMI_PARAM_CONV_W = 0, AZMI_PARAM_BN_WEIGHT = 1, AZMI_PARAM_BN_BIAS = 2, AZMI_PARAM_BN_MEAN = 3, AZMI_PARAM_BN_VAR = 4,
       AZMI_PARAM_FC_W = 5, AZMI_PARAM_FC_B = 6 };
typedef struct azmi_net_param { const void* data; uint64_t count; uint32_t kind; uint32_t reserved; double eps; } azmi_net_param;
int azmi_net_refresh(azmi_net* net, const azmi_net_param* params, uint32_t n_params, void* stream);
/* The live weight image read back into host_out (tests and debugging): synchronises the device.  `bytes` must be the image's size
 * (azmi_net_blob_bytes*): anything else is AZMI_ERR_INVALID and nothing is written; so is a net of the fp32 tier, which keeps its
 * image to itself. */
int azmi_net_blob_read(azmi_net* net, void* host_out, size_t bytes);
/* NNWrapper.process on HOST arrays (neural_net.py:800-823 behind game_runner.py:651-726's batcher -> gpu_loop -> result_worker):
 * canonical [n,C,H,W] -> v [n,P+1], pi [n,M]; copies in, runs the net, copies out, synchronously, on a stream and staging
 * buffers private to the calling thread (any number of host threads may call it at once).  The signature is that of a
 * host PlayManager's evaluator callback (user = the azmi_net*), so a CPU-side PlayManager can be served by the GPU
 * through host buffers without an interpreter in the loop.  Errors are reported by filling v / pi with NaN. */
void azmi_net_eval_host(const float* canonical, uint32_t n, float* v, float* pi, void* net);
/* azmi_net_forward_rows on an engine's own leaf batch and eval list (what azmi_run_rounds does after each round) */
int azmi_pm_net_forward(azmi_pm* pm, azmi_net* net, void* stream);
/* one engine round with its leaf evaluation, as azmi_run_rounds issues it: part 0 = the whole round, 1 = the tree half only
 * (cache insert, simulations), 2 = the net half only (leaf net over the eval list; on the split-round Connect4 engine the
 * round's move step rides in the same launch).  Parts 1 and 2 exist so that a caller can put timing events between them. */
int azmi_pm_round_net(azmi_pm* pm, azmi_net* net, void* stream, uint32_t part);
/* the same for one model group: only the leaves whose seat belongs to `group` (play_manager.cc:577, 597) */
int azmi_pm_net_forward_group(azmi_pm* pm, uint32_t group, azmi_net* net, void* stream);
/* num_model_groups() / num_seat_perms(), play_manager.h:210-211 */
int azmi_pm_groups(azmi_pm* pm, uint32_t* num_model_groups, uint32_t* num_seat_perms);
/* perm_scores(idx) / perm_games_completed(idx), play_manager.h:212-217: out_scores [P+1] */
int azmi_pm_perm_scores(azmi_pm* pm, uint32_t perm, float* out_scores, uint32_t* games_completed);
/* build_batch / update_inferences restricted to one model group (py_wrapper.cc:449-504, play_manager.cc:619-642) */
int azmi_pm_build_batch_group(azmi_pm* pm, uint32_t group, float* batch, uint32_t cap, uint32_t* indices, uint32_t* n);
const char* azmi_net_last_error(void);

/* ---- device position cache on its own: S3FIFOCache / ShardedS3FIFOCache (s3fifo_cache.h:15-318,
 *      Python classes at py_wrapper.cc:222-259).  max_size / ghost_size are totals over `shards`;
 *      shard = hash % shards.  insert_many keeps batch order inside a shard (eviction order is the
 *      reference's); the finds of one call are concurrent.  All pointers are HOST arrays.
 *      stats out[6] = hits, misses, evictions, reinserts, size, max_size. */
int azmi_cache_create(uint32_t max_size, uint32_t shards, uint32_t ghost_size, uint32_t num_policy, uint32_t num_value,
                      int device, azmi_cache** out);
void azmi_cache_destroy(azmi_cache* cache);
int azmi_cache_insert_many(azmi_cache* cache, const uint64_t* hashes, const float* policy, const float* value, uint32_t n);
int azmi_cache_find_many(azmi_cache* cache, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy, float* value);
int azmi_cache_stats(azmi_cache* cache, uint64_t out[6]);
const char* azmi_cache_last_error(void);
/* The same cache on rows that are already in device memory: every pointer below is a DEVICE pointer on the cache's device, the
 * launches are enqueued on `stream` (a HIP stream or NULL) and nothing is read back or waited for.  The only synchronous path is
 * the scratch of the miss list (one prefix per 64 rows, and the list itself for azmi_net_forward_cached): allocated by the first
 * call that needs it and regrown only when a larger n arrives.  A cache is used from ONE stream at a time: two streams on one
 * cache are the caller's to order (an event), as for the host-array entries.  Argument errors are AZMI_ERR_INVALID before any
 * launch, the message (azmi_cache_last_error) naming the argument; n == 0 is AZMI_OK and launches nothing; at most 2^30 rows.
 *   find_rows    S3FIFOCache.find (py_wrapper.cc:226-236 over s3fifo_cache.h:41-59; cache_utils.py:26 `cache.find(h, ...)`) for n
 *                keys: d_hit[i] = 1 / 0; a hit writes rows i of d_pi [n][num_policy] and d_v [n][num_value], a miss leaves them
 *                untouched.  Counters, frequency bump and ghost "reinsert" accounting are azmi_cache_find_many's; hash 0 is a key.
 *                d_miss_rows [n] / d_miss_count [1] (both, or both NULL for no compaction): the rows that missed, ascending, and
 *                their number.  The order is a prefix over hit[], never a ticket: it does not depend on scheduling.
 *   insert_rows  S3FIFOCache.insert (py_wrapper.cc:237-242; cache_utils.py:35 `cache.insert(h, pi, v)`) for the rows
 *                d_rows[0 .. min(*d_row_count, n_max)) of d_keys / d_pi / d_v, in list order: the state
 *                insert_many(keys[rows], pi[rows], v[rows]) leaves (list order is kept inside a shard, s3fifo_cache.h:259-286).
 *                The count is read on the device.  d_rows == NULL: the rows 0 .. n_max - 1 themselves; d_row_count == NULL: n_max.
 *                Every listed index must be a row of the arrays.  ceil(n_max / 8192) launches on 64-entry shards, one otherwise.
 *   azmi_net_forward_cached
 *                cache_utils.cached_inference (cache_utils.py:19-36) for a batch: find_rows, azmi_net_forward_rows over the miss
 *                list, insert_rows over the same list, on one stream.  d_v [n][P+1] and d_pi [n][M] hold every row's answer
 *                afterwards - the cached bits for a hit, the net's for a miss - and d_hit [n] says which.  A key that occurs
 *                several times among the misses of one batch is evaluated every time and inserted once.  Refused: a cache whose
 *                num_policy / num_value are not the net's M / P + 1, a cache on another device than the net. */
int azmi_cache_find_rows(azmi_cache* cache, const uint64_t* d_keys, uint32_t n, uint8_t* d_hit, float* d_pi, float* d_v,
                         uint32_t* d_miss_rows, uint32_t* d_miss_count, void* stream);
int azmi_cache_insert_rows(azmi_cache* cache, const uint64_t* d_keys, const float* d_pi, const float* d_v, const uint32_t* d_rows,
                           const uint32_t* d_row_count, uint32_t n_max, void* stream);
int azmi_net_forward_cached(azmi_net* net, azmi_cache* cache, const float* d_canon, const uint64_t* d_keys, uint32_t n, float* d_v,
                            float* d_pi, uint8_t* d_hit, void* stream);

/* ---- native round driver (the counterpart of GameRunner's batcher / gpu_loop / result_worker
 *      threads, game_runner.py:483-552, 651-726): `rounds` times, for each of the `k` engines in turn:
 *      one round on streams[i], then the net on that engine's slot-indexed leaf batch on the same
 *      stream.  Engines on different streams overlap: while one engine's leaf batch is on the matrix
 *      cores, another engine's tree kernel runs on the CUs the net leaves free.  Launch-only
 *      (asynchronous); poll with azmi_pm_poll. */
int azmi_run_rounds(azmi_pm* const* pms, azmi_net* net, uint32_t k, uint32_t rounds, void* const* streams);
/* ---- asynchronous tree / net pipeline (Connect4 engine; plain PUCT seats + one model group on the fast tree kernel, Gumbel seats and
 *      two model groups on the generic one; bf16 or bf16x3 Connect4-family net): what
 *      azmi_run_rounds does, without its lock step.  The reference's worker loop has no global barrier - every game advances
 *      on its own through the queues between PlayManager::play's workers and GameRunner's batcher threads
 *      (play_manager.cc:258-600, concurrent_queue.h:130-217, game_runner.py:483-552) - and neither has this: for one EPOCH
 *      persistent tree wavefronts simulate their slots and hand the leaves that need the net to persistent net workgroups
 *      (request ring / tagged result granules in HBM, csrc/pipe_types.h); an epoch ends after `sims_per_epoch` simulations
 *      (held to 1024 per slot; an epoch also ends a quarter of the way to the 250 ms stall cap, or when an eighth of the slots'
 *      games have ended in it), then game restarts, the moves the epoch's end cut off and the position-cache inserts of its answers
 *      run at a kernel boundary.  A slot lives in ONE tree workgroup (slot % tree workgroups) for an epoch - searches AND moves -, so
 *      nothing but requests, answers and READY tokens crosses between CUs inside an epoch.  `epochs` epochs, synchronous (returns
 *      when they are done).  net == NULL: an engine whose seats all use EvalType::RANDOM runs on the tree kernel alone.
 *      A pipeline error (a spin that hit the time cap: another tenant holds the chip, the host stalled between the two launches)
 *      is reported here ONCE and cleared: slots whose requests went unanswered are back in the move step's kSlotQueued form, so
 *      the next call of either driver carries on.  The k-th game of a slot is that of azmi_run_rounds for the same seed; with a finite
 *      games_to_play, WHICH slots receive the last restarts depends on the order in which games end inside an epoch (as the reference's
 *      workers race for games_started_, play_manager.cc:506-513), so the SET of games is only the same while no game restarts.
 *      out_stats[14] = the calibration launches of this call (bits 0-7) | freezes - tree wavefronts that stood still for more than
 *      2 ms between two looks of their poll loop (seen with hundreds of idle net workgroups beside a small engine);
 *      credited against the time caps, not errors - since creation (bits 8-31) | requests given up and sent again since creation
 *      (bits 32-63).  An epoch launches min(the measured places, S / 3 + 8) net workgroups: a slot has at most one request out and
 *      a tile takes three.
 *      Worst case of ONE epoch: the tree side's stall detector is the 250 ms cap (AZMI_PIPE_CAP_MS); the net side only waits for
 *      the tree side and outwaits it for 40 caps = 10 s before it raises error bit 64 itself - a tree kernel that never starts
 *      (the host held up between the two launches, no place on the chip) is an error after 10 s, not a hang.  A net workgroup beyond
 *      the S / 3 + 8 the slots can use (only launched under AZMI_PIPE_NET_ALL) that idles beside a tree side without progress for
 *      1.25 caps leaves instead.
 *      out_stats (may be NULL): [0] net tiles run since the pipeline was created, [1] boards in them, [2] simulations of the
 *      last epoch, [3] / [4] tree / net workgroups that started in it, [5] its insert-log entries, [6] / [7] net / tree
 *      workgroups launched, [8] / [9] the latest start of a tree / net workgroup after the epoch's first, in microseconds (all
 *      of them must be on the chip together: a late one found its place only when another left), [10] / [11] the summed
 *      durations of this call's net / tree kernels in microseconds (HIP events on their streams), [12] the epochs of this
 *      call, [13] the host time spent enqueueing them in microseconds (the host runs ahead of the GPU), [14] the calibration
 *      launches that measured [6] (0 = not measured: tree side alone); 16 entries.
 *      After azmi_pm_stop both this call and azmi_run_rounds return AZMI_OK at once and run nothing (play_manager.cc:272). */
int azmi_run_pipeline(azmi_pm* pm, azmi_net* net, uint32_t epochs, uint64_t sims_per_epoch, void* stream, uint64_t* out_stats);
/* the same with one net PER MODEL GROUP (azmi_run_rounds_groups' counterpart: play_past, game_runner.py:2184-2332 - two models, seats
 * swapped by the permutations): nets[g] evaluates the leaves of group g (its own request ring, its own S3-FIFO), NULL = that group
 * needs no net (RANDOM seats: the reference's RandPlayer).  At most two groups; every net a Connect4-family matrix-core net of ONE
 * precision tier.  Engines the fast tree kernel does not cover - Gumbel seats, two model groups - run on the generic tree kernel
 * (every step through the lock-step engine's own move-step function, one simulation per slot and pass, no round barrier). */
int azmi_run_pipeline_groups(azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets, uint32_t epochs, uint64_t sims_per_epoch, void* stream,
                             uint64_t* out_stats);
int azmi_pipeline_supported_groups(azmi_pm* pm, azmi_net* const* nets, uint32_t num_nets);
/* diagnostics: the pipeline's persistent net kernel alone, draining `n` synthetic requests (n <= 32768, the request ring) `reps` times with
 * `net_wgs` workgroups (0 = the pipeline's own count) and tile selection `mode` (0 = 3- and 6-board tiles, 1 = 6-board, 2 =
 * 3-board; 3 was a removed experiment's net side and is an AZMI_ERR_STATE error); *ms_out = milliseconds per drain.  Timing only
 * (scripts/pipe_net_timing.py -> profiles/). */
int azmi_debug_pipe_net_bench(azmi_pm* pm, azmi_net* net, uint32_t n, uint32_t reps, uint32_t net_wgs, int mode, float* ms_out);
/* diagnostics: out[0] = answers the tree side consumed in the last epoch of the last azmi_run_pipeline call (its insert log), out[1] =
 * those whose key is in the log more than once (evaluations an insert at answer time - PlayManager::update_inferences,
 * play_manager.cc:631-640 - or a table of requests in flight would have saved), out[2] = of those, twins within 4096 log entries */
int azmi_debug_pipe_log_dupes(azmi_pm* pm, uint64_t* out);
/* diagnostics: the descent's lane-group primitives on their own, one wavefront (eight 8-lane groups) per row.  Inputs per group
 * (rows x 8): k, v_parent, n_parent, fpu, cpuct; per lane (rows x 64, lane j of group g at 8 g + j): n_l, q_l, p_l; pred[row]: a 64-bit
 * lane predicate.  Outputs per lane (rows x 64): sum64 = the in-order sum of the priors of the visited children as that lane holds
 * it, best64 = select_child's winner, all64 = bit 0: every lane of the group has its predicate bit set, bit 1: some lane has.
 * tests/test_gpu_group_primitives.py */
int azmi_debug_group_select(int device, uint32_t rows, const uint32_t* k8, const uint32_t* n64, const float* q64, const float* p64,
                            const float* v_parent8, const uint32_t* n_parent8, const float* fpu8, const float* cpuct8, const uint64_t* pred,
                            float* sum64, uint32_t* best64, uint32_t* all64);
/* diagnostics: expand_node (Node::add_children, mcts.cc:93-101) on its own, in the form of the lock-step kernels (lane_pack = 0) or of
 * the pipeline's tree kernel (lane_pack = 1: the move word is packed by the group's lanes).  One wavefront per row; each of its eight 8-lane groups
 * expands `reps` Connect4 positions one after the other into tree 0 of its own slot (slot = 8 row + group; `cap` nodes per tree, nodes
 * 0 .. reps-1 are the parents, children are appended behind them).  Inputs per call (rows x 8 x reps, call r of slot s at s reps + r):
 * the two bitboards, the player to move, the RNG state the call starts from.  Outputs per lane of a call ((s reps + r) 8 + lane):
 * words[4] = the lane's child move, c0, k, 1 when the arena had room; rng_out = the RNG state afterwards; nodes_out = the arena
 * (rows x 8 slots x 2 trees x cap records of 32 bytes: u32 n, f32 q, pr, d, v, u32 unused, u64 meta), prefilled with 0xAB bytes.
 * tests/test_gpu_group_expand.py */
int azmi_debug_group_expand(int device, uint32_t lane_pack, uint32_t rows, uint32_t reps, uint32_t cap, const uint64_t* bb0, const uint64_t* bb1,
                            const uint32_t* player, const uint64_t* rng_in, uint32_t* words, uint64_t* rng_out, void* nodes_out);
/* diagnostics: out[i] = the cache shard of hashes[i] among `shards` (hash % shards, computed the way the kernels compute it: a
 * multiply by a constant of the cache and one correction).  device < 0: the host's compilation, no GPU needed; otherwise one
 * thread per hash on that device.  tests/test_shard_index.py */
int azmi_debug_shard_index(int device, uint32_t shards, const uint64_t* hashes, uint32_t n, uint32_t* out);
/* diagnostics: azmi_cache_find_many on a cache of 64-entry wave shards, probing with wave_shard_find<group_lanes> - the lane groups the
 * engines probe with (GM::GROUP: 8 and 64); the stand-alone call always uses 8.  Same accounting, same outputs.  Other values of
 * group_lanes and caches in another layout are errors (azmi_cache_last_error).  tests/test_gpu_cache_edges.py */
int azmi_debug_cache_find_group(azmi_cache* cache, uint32_t group_lanes, const uint64_t* hashes, uint32_t n, uint8_t* hit, float* policy,
                                float* value);
/* diagnostics: the pipeline's cache insert (one wavefront per entry under the shard's insert lock, wave_shard_insert_locked) on host
 * arrays: ONE kernel in which `waves` wavefronts (1 .. 8192) stride over the n entries, with a zeroed lock word per shard allocated
 * for the call.  waves = 1 inserts in batch order.  *failed_out = the entries whose lock was not had (0 unless something is wrong).
 * Needs 64-entry wave shards and num_policy, num_value <= 64 (azmi_cache_last_error otherwise). */
int azmi_debug_cache_insert_locked(azmi_cache* cache, const uint64_t* hashes, const float* policy, const float* value, uint32_t n,
                                   uint32_t waves, uint32_t* failed_out);
/* 1 when azmi_run_pipeline can drive this engine with this net (net may be NULL for an engine whose seats all use
 * EvalType::RANDOM: the tree kernel alone), 0 otherwise (then azmi_run_rounds is the driver) */
int azmi_pipeline_supported(azmi_pm* pm, azmi_net* net);
/* the same loop with one net per MODEL GROUP (gating / benchmark matches between two models, game_runner.py:2184-2332):
 * nets[g] evaluates the leaves of group g, NULL = the group needs no net (RANDOM / PLAYOUT evaluator) */
int azmi_run_rounds_groups(azmi_pm* const* pms, azmi_net* const* nets, uint32_t num_nets, uint32_t k, uint32_t rounds, void* const* streams);

/* ---- the path's one exchange step: finished self-play samples go to rank 0 over RCCL / xGMI ---------------------------
 * Replaces the reference's hist_saver (game_runner.py:729-747: one process, a queue) for one process per GPU.  No collective runs
 * during the search.  librccl is loaded (dlopen) by the first of these calls; a one-GPU process that never gathers does not need it.
 *   azmi_comm_available  AZMI_OK when librccl and every entry point used here load in this process (no communicator is made): what
 *                        the ranks agree on BEFORE any of them enters ncclCommInitRank - a rank that would fail there strands the
 *                        others inside it
 *   azmi_comm_unique_id  rank 0: the 128 bytes every rank passes to azmi_comm_create (carried there by the launcher's own channel:
 *                        bench.py broadcasts them with torch.distributed)
 *   azmi_comm_create     ncclCommInitRank on `device`
 *   azmi_gather_counts   every rank: its row count in, all ranks' counts out (one ncclAllGather of 8 bytes per rank; synchronises
 *                        `stream`)
 *   azmi_gather_rows     every rank: `num_parts` device arrays of counts[rank] rows, row_bytes[i] bytes per row; rank 0 receives them
 *                        in rank order, unpadded, into dst[i] (device memory for sum(counts) rows; ignored on the other ranks):
 *                        grouped ncclSend / ncclRecv, its own rows by a device copy.  Asynchronous on `stream`. */
typedef struct azmi_comm azmi_comm;
int azmi_comm_available(void);
int azmi_comm_unique_id(void* out128);
int azmi_comm_create(const void* id128, int rank, int world, int device, azmi_comm** out);
void azmi_comm_destroy(azmi_comm* comm);
int azmi_gather_counts(azmi_comm* comm, uint64_t n_local, uint64_t* out_counts, void* stream);
int azmi_gather_rows(azmi_comm* comm, const void* const* src, const uint64_t* row_bytes, uint32_t num_parts, const uint64_t* counts,
                     void* const* dst, void* stream);

/* The device RNG layer on its own (parity tier "RNG"): runs `thread_local pcg32 re` + the
 * libstdc++ algorithm the reference applies to it (mcts.cc:19,100,430-440,718) on the GPU.
 * kind 0: n raw pcg32 outputs (u32)      1: std::shuffle of iota(n), reps times (u32 [reps,n])
 *      2: n uniform_real<float>(0,1)      3: n gamma_distribution<float>(param,1), one object
 *      4: same, a fresh object per draw.  `out` is a HOST array of n (kind 1: reps*n) 4-byte items. */
int azmi_rng_probe(int device, int kind, uint64_t seed, float param, uint32_t n, uint32_t reps, void* out);

#ifdef __cplusplus
}
#endif
#endif /* AZMI_H_ */
