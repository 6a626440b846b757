// C-ABI of libmds (include/mds.h): handle management, constant set-up in double, dtype
// dispatch and kernel launches.  No torch types, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/mds.h"
#include "mds_consts.hpp"
#include "mds_devmem.hpp"
#include "mds_kernels.hip"
#include "mds_traj_image.hpp"
#ifndef MDS_PART
#define MDS_PART 3
#endif
#if MDS_PART & 1
#include "mds_episode_kernels.hip"  // per-env episodes inside the rollout kernel (part 1 only)
#include "mds_episode_policy_kernels.hip"   // ... driven by an MLP policy evaluated in the kernel (part 1 only)
#include "mds_episode_sample_kernels.hip"   // ... whose actions are drawn from a Gaussian around its output (part 1 only)
#endif
#if MDS_PART & 2
#include "mds_cbf_kernels.hip"      // (part 2 only: it defines a non-template kernel)
#include "mds_fedce_kernels.hip"    // FedCE identification and the dLQR kernels (part 2 only)
#include "mds_fedce_omega_kernels.hip"   // the same on the 9-state thrust / body-rate model (part 2 only)
#include "mds_care_kernels.hip"     // the Riccati solver of both models' dLQR gains (part 2 only)
#else
#include "mds_cbf.hpp"
#endif

using namespace mds;

// The library builds as one translation unit (MDS_PART 3, the default: `hipcc -shared mds_api.hip`) or as two compiled side by
// side and linked (__graft_entry__.build(): -DMDS_PART=1 = handle management, the step / rollout / conversion entry points;
// -DMDS_PART=2 = the ECBF filter, the LQR / DSLPID / low-level controllers and the CBF rollouts) -- the device code of ~200 kernel
// instantiations compiles serially per unit, so two units halve the build and a change to the CBF kernels rebuilds one of them.
namespace mds_detail {
extern thread_local char g_err[512];            // last error text of the calling thread (mds_last_error): one copy for both parts
#if MDS_PART & 1
thread_local char g_err[512] = "";
#endif
}  // namespace mds_detail
using mds_detail::g_err;

namespace {


int fail_hip(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return MDS_EHIP;
}
int fail(int code, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}
int fail(int code, const char* who, const char* what) {          // "<entry point><what>": checks shared by several entry points
  snprintf(g_err, sizeof(g_err), "%s%s", who, what);
  return code;
}

#define MDS_HIP(call)                          \
  do {                                         \
    hipError_t e__ = (call);                   \
    if (e__ != hipSuccess) return fail_hip(e__, #call); \
  } while (0)

// The one binding of the handle's allocator (mds_devmem.hpp) to the HIP runtime: every block a handle owns is allocated, zero-filled
// and freed here and nowhere else.  Out of device memory is MDS_ENOMEM from every entry point, any other failure MDS_EHIP.
int dev_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return MDS_OK;
  return e == hipErrorOutOfMemory ? fail(MDS_ENOMEM, what, ": out of device memory") : fail_hip(e, what);
}
const DevAllocator kHipAllocator = {
    [](void** out, size_t bytes) { return dev_status(hipMalloc(out, bytes), "hipMalloc"); },
    [](void* p) { (void)hipFree(p); },
    [](void* p, size_t bytes) { return dev_status(hipMemset(p, 0, bytes), "hipMemset"); },
};

size_t elem_size(int dtype) { return dtype == MDS_F64 ? 8 : (dtype == MDS_F16 ? 2 : 4); }   // MDS_F32C: fp32 buffers
size_t comp_size(int dtype) { return dtype == MDS_F64 ? 8 : 4; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Every entry point runs with the handle's device current and restores the caller's on return: a process may hold
// handles on several GPUs (one env per device, or a trajectory-evaluation handle next to an env), and neither the
// launches nor the set-up allocations may land on whatever device the calling thread happened to have selected.
struct DevGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DevGuard(int dev) {
    if (dev < 0) return;
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = err == hipSuccess;
    }
  }
  ~DevGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};
#define MDS_DEV(h) DevGuard dev_guard__((h) ? (h)->cfg.device : -1)

__global__ void k_noop() {}


}  // namespace

// Everything the host prepares once per compute type T and passes to kernels by value.  The handle keeps a float and a double instance
// (params<T>(h)): the setters fill both, a launch takes the one of its dtype.
template <typename T> struct HostParams {
  Consts<T> c;
  EnvFx<T> fx;
  CbfParams<T> cbf;
  DslPidGains<T> pid;
  LqrGain<T> lqr;
  LqrYoGain<T> lqr_yo;
  Lqr12Gain<T> lqr12;
};

struct mds_handle {
  explicit mds_handle(const DevAllocator& a) : mem(a) {}
  DevMem mem;                    // owner of every device block behind the pointer fields below: they are allocated and freed through it alone
  mds_config cfg = {};
  mds_geometric_gains gains = {};
  double wind[3] = {0.0, 0.0, 0.0};
  int n = 0;
  size_t ld = 0;                 // plane stride (elements)
  void* state = nullptr;         // S [13][ld]
  void* state_lo = nullptr;      // MDS_F32C: float [ld][4] = residuals of the three body rates + pad (load_resid in mds_kernels.hip)
  void* origin = nullptr;        // T [3][ld]
  void* last_rpm = nullptr;      // T [4][ld]
  void* lem = nullptr;           // T [7][ld]
  double* scratch = nullptr;     // double [n*20] device staging for host<->device set-up calls
  double* init_pose = nullptr;   // double [n*6]: xyz, rpy of the last mds_reset (episode resets on the device, mds_reset_async)
  bool has_traj = false;
  int traj_mode = 0;             // 1: per-drone Lemniscate planes (fused fp32 fast path), 2: general segment tables
  bool traj_yaw_free = false;    // every Lemniscate of the last upload has yaw_rate = +-0 (mds_set_lemniscate; segment tables: false)
  bool traj_spec = true;         // mds_set_traj_specialisation: such a handle steps through the yaw-free kernels
  // the phase table of the whole-rollout loop (k_rollout_geometric_y0p): sin / cos of the Lemniscate phases, one row of 64 pairs per step
  bool traj_phase_periodic = false;   // the last upload's (omega, phase_shift) repeat every 64 drones (lemniscate_phase_periodic; segment tables: false)
  bool phase_tab_on = true;      // mds_set_traj_phase_table
  void* phase_tab = nullptr;     // T [kPhaseTabRows][64][2] (pairs) or [kPhaseTabRows][2][64][4] (wide rows), allocated by the first upload that qualifies
  bool phase_tab_filled = false; // the rows hold the steps of a flight; an upload clears it
  int phase_tab_rows = 0;        // how many rows the last fill wrote
  int phase_tab_row = 0;         // the row of the step that follows the last launch served ...
  double phase_tab_t = 0.0;      // ... and its time: a launch that starts there, to the bit, goes on reading; any other refills from row 0
  int last_rollout_phase_table = 0;   // the last whole-rollout launch read the table (mds_get_last_rollout_phase_table)
  // the desired-state table (k_rollout_geometric_y0d): the same block and bookkeeping, rows of 64 x 8 values (LemDesired8)
  bool traj_desired_periodic = false; // the last upload's a repeats every 64 drones as well (lemniscate_desired_periodic; segment tables: false)
  bool desired_tab_on = true;         // mds_set_traj_desired_table
  size_t phase_tab_bytes = 0;         // the size of the block: narrow rows (1 MB) or wide ones (4 MB, serves either layout)
  bool phase_tab_wide = false;        // the layout of the rows the last fill wrote
  int last_rollout_desired_table = 0; // ... and it read wide rows (mds_get_last_rollout_desired_table)
  double* segs = nullptr;        // device [MDS_SEG_DIM, total]: field-major (mds_traj.hpp SegTable)
  int nseg_total = 0;
  int* tinfo = nullptr;          // device [n, 3] = first segment, nseg | compound << 16, stride between pieces (mds_traj.hpp TrajInfo)
  HostParams<float> p32 = {};
  HostParams<double> p64 = {};
  // ECBF filter
  bool has_cbf = false;
  mds_cbf_params cbf = {};
  int* pair_ij = nullptr;        // device [D(D-1)/2]
  void* obstacles = nullptr;     // device T [n_obs,4]
  // slot 0: the whole batch; slots 1, 2: the two env halves of mds_rollout_cbf_geometric (each keeps its own cost classes)
  int* cbf_order = nullptr;      // [3 slots][3,E] env ids by cost class (longest-first dispatch of the QP kernel)
  int* cbf_count = nullptr;      // [3 slots][4]
  int cbf_calls_half[2] = {-1, -1};
  int* cbf_cost = nullptr;       // [E] GI iterations of the last launch
  int cbf_calls = -1;            // launches since the classes were rebuilt; -1: no classes yet
  int rollout_streams = 0;              // mds_set_rollout_streams: 0 auto, 1, 2
  // two-chain rollouts: chain 0 runs on the caller's stream, chain 1 on this internal stream; ev[0] forks it off the caller's
  // stream, ev[1] joins it back.  Created (and primed) by mds_create for shards that can split, else by mds_set_rollout_streams(h, 2).
  hipStream_t split_st = nullptr;
  hipEvent_t split_ev[2] = {nullptr, nullptr};
  int last_rollout_streams = 0;         // what the last mds_rollout_* call did (mds_get_last_rollout_streams)
  int rollout_form = 0;                 // mds_set_rollout_form: 0 auto, 1 one launch per control step, 2 the whole-rollout kernel in chunks
  int rollout_chunk = 50;               // control steps per launch of form 2
  int last_rollout_form = 0;            // what the last mds_rollout_geometric did (mds_get_last_rollout_form)
  bool next_nom_ok[3] = {false, false, false};   // per env-range slot: the last low-level launch also left the nominal input of ...
  double next_nom_t[3] = {0.0, 0.0, 0.0};        // ... the control step at this time in the scratch (C rollout loops chain on it)
  bool cbf_hildreth = false;            // MDS_CBF_SOLVER=hildreth, read once by mds_cbf_configure
  bool cbf_q4 = false;                  // MDS_CBF_Q4=1 at configure time: the four-envs-per-wave QP kernel (k_cbf_filter_q4) where it applies; measured
                                        // no faster than one env per wave (see its header), so opt-in
  int cbf_last_step_kernel = -1;        // what the most recent CBF-filtered step launched: 1 the one-launch kernel, 0 QP + low level
  bool cbf_step_persistent = false;     // mds_cbf_set_step_kernel(h, 2): a CBF-filtered step = one launch of the persistent rollout kernel where it applies
  bool cbf_fused = false;               // mds_cbf_set_step_kernel / MDS_CBF_FUSED=1 at configure time: the one-launch CBF step (k_cbf_step) where it applies; it wins only
                                        // on scenes whose QPs need no iterations (see the kernel's header), so the default is the three launches
  void* cbf_unom = nullptr;      // S [n,4]  scratch of mds_step_cbf_geometric
  void* cbf_xdes = nullptr;      // S [n,9]
  void* cbf_usafe = nullptr;     // S [n,4]
  void* ll = nullptr;            // T [6][ld]: ThrustOmega last_omega3 | integral3
  void* pid = nullptr;           // T [9][ld]: DSLPID last_rpy3 | integral_pos_e3 | integral_rpy_e3
  bool has_lqr = false;
  int cbf_nominal = 0;           // 0 geometric, 1 lqr-omega, 2 lqr-yank-omega (order 3), 3 dlqr-omega (coupled over the env's drones)
  bool has_lqr_yo = false;
  bool has_lqr12 = false;
  // device copies of the gains for the whole-rollout kernels: 0 LQR-12, 1 LQR-omega, 2 LQR-yank-omega (written by the mds_set_*_gain calls)
  void* gain_dev[3] = {nullptr, nullptr, nullptr};
  void* state_alt = nullptr;     // second state buffer of the ground-effect / downwash step (double-buffered substeps)
  void* act_scratch = nullptr;   // S [n,4]: the controller's action, replayed by the later substeps of a ground-effect / downwash step
  bool envfx = false;            // physics has ground effect and / or downwash
  // FedCE / dLQR (mds_fedce_*, mds_*dlqr*): per-drone RLS state in float64, per-env gain in the compute type
  double* fedce_P = nullptr;      // [n][16][16]
  double* fedce_theta = nullptr;  // [n][12]: the free entries of theta (mds_fedce_kernels.hip)
  void* dlqr_K = nullptr;         // T [E][4][12 D][D] (dlqr_kidx)
  // the 9-state learner (mds_fedce_omega_*, mds_*dlqr_omega*): information matrix V, W = V^-1 and the full theta, float64
  double* fo_V = nullptr;         // [n][13][13]
  double* fo_W = nullptr;         // [n][13][13]
  double* fo_theta = nullptr;     // [n][13][9]
  void* dlqr_omega_K = nullptr;   // T [E][4][9 D][D] (dlqr_kidx_m<9>)
  // the device Riccati solver (mds_dlqr_solve_gain / mds_dlqr_omega_solve_gain), slot 0: 12-state, 1: 9-state
  double* care_tab[2] = {nullptr, nullptr};      // R^-1 [D][16] | Q of every single [M, M] | Q of every pair [2M, 2M]
  std::vector<double> care_tab_host[2];          // what care_tab holds: a call with the same Q and R uploads nothing
  double* care_K64[2] = {nullptr, nullptr};      // [E, 4D, MD] float64 staging when the caller passes no K_dev
  bool track_rpm = false;        // last_rpm planes maintained by every step kernel (DYN_DRAG, order-3 CBF, or cfg.track_last_rpm)
  bool rpm_stale = false;        // a step ran without tracking since the last reset
  // per-env episodes (mds_set_episodes): the rule, the reset image k_reset wrote (layout and dtype of `state`), the targets and the counters
  bool ep_on = false;
  mds_episode_params ep = {};
  void* ep_image = nullptr;            // S [13][ld]
  void* ep_target = nullptr;           // T [4][ld]: three planes of local-frame targets (the fourth: k_reset's RPM planes while the image is built)
  double* ep_target_world = nullptr;   // double [n,3]: the caller's targets; NULL: the reset positions
  void* ep_counters = nullptr;         // five arrays of 8-byte slots, [ep_slots] each: length | ret | count | sum_return | sum_length
  size_t ep_slots = 0;
  // collision causes of the episodes (mds_set_episode_safety): the set as the caller gave it, and the env's smallest h
  bool ep_safe = false;
  mds_episode_safety ep_safety = {};
  double ep_obstacles[4 * MDS_EPISODE_MAX_OBSTACLES] = {};
  void* ep_hmin = nullptr;             // two arrays of 8-byte slots, [ep_slots] each: h_min_step | h_min_episode (compute type)
  // randomised episode starts (mds_set_episode_randomisation): the parameters as the caller gave them (they travel to the kernels by
  // value) and the generation word of the draw, 0 at configuration, + 1 with every mds_reset_episodes
  bool ep_random = false;
  mds_episode_randomisation ep_rand = {};
  uint32_t ep_generation = 0;
  // the MLP policy of the episodes (mds_set_episode_policy): the parameters with the defaults resolved, and the weights in the compute
  // type, zero-padded to ep_policy_width (one of kPolicyWidths)
  bool ep_policy = false;
  mds_episode_policy ep_pol = {};
  int ep_policy_width = 0;
  void* ep_policy_w = nullptr;
  // the Gaussian noise of the policy's actions (mds_set_episode_policy_noise) and the epoch word of its draw: 0 at configuration, + 1
  // with every host call that restarts every env's running episode
  bool ep_noise = false;
  mds_episode_policy_noise ep_noise_p = {};
  uint32_t ep_epoch = 0;
};

template <typename T> static inline const HostParams<T>& params(const mds_handle* h) {
  if constexpr (sizeof(T) == 8) return h->p64;
  else return h->p32;
}

static inline bool has_drag(const mds_handle* h) {
  return h->cfg.physics == MDS_PHYSICS_DYN_DRAG || h->cfg.physics == MDS_PHYSICS_DYN_GND_DRAG_DW;
}

// The last clipped action lives in the obs a step call returns.  The SoA copy costs 16 B per drone-step
// and is kept only where something reads it back (the _drag term, calc_z_thrust of the yank path, mds_get_obs).
static inline void* rpm_track(mds_handle* h) {
  if (h->track_rpm) return h->last_rpm;
  h->rpm_stale = true;
  return nullptr;
}

// Shards at least this large step their two halves on two streams inside mds_rollout_geometric (0 = auto policy).
constexpr size_t kSplitMinDrones = size_t(1) << 18;
// Calls shorter than this stay on the caller's stream under the auto policy: a two-chain call costs a fork and a join (two
// cross-stream dependencies) and its halves start in lock step -- ~35 us more than n x its steady-state step.  C3, wall-clock us
// per control step (enqueue .. synchronize, median of 21 calls) by call length, one stream -> two chains: 8 steps 20.3 -> 20.8,
// 12 steps 19.0 -> 19.0, 16 steps 19.0 -> 18.1, 20 steps 18.7 -> 17.7, 32 steps 18.2 -> 16.9, 48 steps 18.0 -> 16.5; by HIP events
// 100 steps 17.4 -> 15.2, 2000 steps 17.4 -> 14.8 (profiles/r02_short_calls.log).
constexpr int kSplitMinSteps = 16;
// LDS bytes a half-shard workgroup occupies in a two-chain rollout: its launch carries unused dynamic LDS up to this
// (step_geometric says why)
constexpr size_t kSplitLds = 32768;

// The stream policy in one place (mds_set_rollout_streams; mds_rollout_streams_for reports it).  loop 0: the fused geometric /
// plain env.step loops (size sweep of DESIGN.md 4: below 2^18 drones the extra launches cost more than the overlap gains,
// between 2^18 and 2^19 it pays only once the chains have had ~1000 steps to drift out of phase); loop 1: the CBF loop
// (2^15 drones 36.6 vs 36.4 us, 2^16 41.0 vs 39.4, 2^17 52.9 vs 44.7, 2^18 71.7 vs 60.3).
static int rollout_streams_policy(const mds_handle* h, int loop, int n_steps) {
  if (n_steps < 2 || !h->split_st || h->envfx) return 1;     // ground effect / downwash: the substeps swap two state buffers, one chain
  if (h->rollout_streams) return h->rollout_streams;
  const size_t n = (size_t)h->n;
  if (loop == 1) return (n >= kSplitMinDrones / 4 && n_steps >= kSplitMinSteps) ? 2 : 1;
  const bool big = n >= 2 * kSplitMinDrones ? n_steps >= kSplitMinSteps : (n >= kSplitMinDrones && n_steps >= 1000);
  return big ? 2 : 1;
}

// The launch form of the fused geometric loop (mds_set_rollout_form; mds_rollout_form_for reports it).  1: one launch per control step
// (k_step_geometric; two chains on big shards, above).  2: the whole-rollout kernel in launches of `rollout_chunk` control steps
// (k_rollout_geometric: state in registers, every step's observation still written).  Auto: form 2 for every shard of kFusedMinDrones drones
// and more and calls of kFusedMinSteps steps and more -- it is the faster form at every size measured (profiles/r04_shard_sweep.json,
// r04_form_sweep.json): below 2^18 drones form 1 is launch-bound (a dependent launch costs ~4 us whatever it moves: C2, 16 384 drones, 3.9 us
// per step against 1.9; one eighth of config 3, 65 536 drones, 4.75 against 1.97), above it form 1 streams the 13-value state through HBM
// twice per step (212 B per drone-step at 0.8-0.93 of the roofline: config 3 15.4 us per step) where form 2 moves the observation row only
// (82.6 B: 7.5-9.0 us, VALU-bound).  float64 likewise (config 3: 32.7 -> 30.9 us per step, 4 M drones 330 -> 246; its whole-rollout kernel is
// arithmetic-bound -- software sin / cos / atan2 / asin, divisions -- and wins by less).  fp16 storage stays in form 1 (form 2 rounds the
// state to fp16 once per launch instead of once per step: not the same arithmetic).
constexpr size_t kFusedMinDrones = size_t(1) << 13;
constexpr int kFusedMinSteps = 8;
static int rollout_form_policy(const mds_handle* h, int n_steps) {
  if (h->envfx || n_steps < 1) return 1;          // ground effect / downwash: env-mates interact every substep, no state-in-registers form
  if (h->rollout_form) return h->rollout_form;
  if (h->cfg.dtype == MDS_F16) return 1;
  return ((size_t)h->n >= kFusedMinDrones && n_steps >= kFusedMinSteps) ? 2 : 1;
}

// Set-up path (mds_create / mds_set_rollout_streams): the internal stream and the two events of the two-chain rollouts.
// The new stream runs one empty kernel and is drained, so that its hardware queue exists and has dispatched before any
// rollout uses it -- the rollouts themselves never create or initialise anything (mds.h: hot-path calls only enqueue).
static int split_streams_ready(mds_handle* h) {
  if (h->split_st && h->split_ev[0] && h->split_ev[1]) return MDS_OK;
  if (!h->split_st) {
    // ROCm multiplexes a process's streams onto GPU_MAX_HW_QUEUES (4 by default) hardware queues; when the caller's stream and this one share
    // a queue the two chains serialise (C4 with 8 other active streams in the process: 49 -> 87 us per step).  A stream of another priority
    // level lives on queues of its own: MDS_SPLIT_STREAM_PRIORITY=high|low is for such applications (no measurable cost or gain otherwise).
    const char* pe = getenv("MDS_SPLIT_STREAM_PRIORITY");          // read per stream creation (per handle), as mds.h says
    const int prio_mode = !pe ? 0 : (pe[0] == 'h' || pe[0] == '1') ? 1 : (pe[0] == 'l' || pe[0] == '2') ? 2 : 0;
    if (prio_mode) {
      int lo = 0, hi = 0;
      MDS_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
      MDS_HIP(hipStreamCreateWithPriority(&h->split_st, hipStreamNonBlocking, prio_mode == 1 ? hi : lo));
    } else {
      MDS_HIP(hipStreamCreateWithFlags(&h->split_st, hipStreamNonBlocking));
    }
    k_noop<<<1, 64, 0, h->split_st>>>();
    MDS_HIP(hipGetLastError());
  }
  for (int k = 0; k < 2; ++k)
    if (!h->split_ev[k]) MDS_HIP(hipEventCreateWithFlags(&h->split_ev[k], hipEventDisableTiming));
  MDS_HIP(hipEventRecord(h->split_ev[1], h->split_st));
  MDS_HIP(hipStreamSynchronize(h->split_st));
  return MDS_OK;
}

// Entry / exit of a two-chain rollout (step_loop below is their one caller).  Chain 0 is the caller's stream itself: its launches
// wait for nothing, and the call costs two cross-stream dependencies in all (four, and 50 us per call, when both chains ran on
// internal streams).
// fork: the internal stream waits for everything enqueued on the caller's stream so far.
// join: the caller's stream waits for chain 1 -- step_loop runs it whenever it has attempted the fork, also when the fork itself or
// a launch in between failed, so that the caller's stream keeps ordering whatever was enqueued (mds.h: the caller's stream orders
// the whole call).
static int split_fork(mds_handle* h, hipStream_t st) {
  MDS_HIP(hipEventRecord(h->split_ev[0], st));
  MDS_HIP(hipStreamWaitEvent(h->split_st, h->split_ev[0], 0));
  return MDS_OK;
}
static int split_join(mds_handle* h, hipStream_t st, int rc_body) {
  int rc = rc_body;
  hipError_t e = hipEventRecord(h->split_ev[1], h->split_st);
  if (e == hipSuccess) e = hipStreamWaitEvent(st, h->split_ev[1], 0);
  if (e != hipSuccess && rc == MDS_OK) rc = fail_hip(e, "two-chain rollout: join");
  return rc;
}

static int check_launches() {
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

// One step chain of a per-step rollout: its stream and the part [i0, i0 + n) of the shard it steps, in the caller's unit (256-drone
// batches; envs in the CBF loop).  n == 0: the whole shard, launched as a single step call launches it.
struct Chain {
  hipStream_t st;
  unsigned i0, n;
};

// envs [e0, e0 + ne) of the batch; slot selects the cost-class tables (0: whole batch, 1 / 2: halves of a two-stream rollout)
struct EnvRange {
  int e0, ne, slot;
};

// The driver of every one-launch-per-control-step rollout.  Control steps [k_first, n_steps) go through step(k, chains, n_chains),
// called once per step: it enqueues the step on chain 0, then on chain 1, and advances whatever it carries from step to step (the
// time, ring indices) once.  streams == 2 (rollout_streams_policy) with a shard that has a middle makes two chains: [0, mid) on the
// caller's stream, [mid, total) on the internal one, forked before the first launch and always joined.  Only enqueues.
template <typename Step>
static int step_loop(mds_handle* h, hipStream_t st, int streams, unsigned mid, unsigned total, int k_first, int n_steps, Step& step) {
  const bool two = streams == 2 && mid > 0;
  const Chain chains[2] = {{st, 0, two ? mid : 0}, {h->split_st, mid, total - mid}};
  h->last_rollout_streams = two ? 2 : 1;
  int rc = two ? split_fork(h, st) : MDS_OK;
  for (int k = k_first; k < n_steps && rc == MDS_OK; ++k) rc = step(k, chains, two ? 2 : 1);
  if (rc == MDS_OK) rc = check_launches();
  return two ? split_join(h, st, rc) : rc;
}
// the same for the loops over 256-drone batches: two chains when the policy says so and the shard has two batches
template <typename Step> static int step_loop_batches(mds_handle* h, hipStream_t st, int k_first, int n_steps, Step& step) {
  const unsigned nbatch = (unsigned)((h->n + kBlock - 1) / kBlock);
  return step_loop(h, st, rollout_streams_policy(h, 0, n_steps), nbatch / 2, nbatch, k_first, n_steps, step);
}

// A rollout in launches of at most per_launch control steps: launch by launch, the step it starts at (k), its time -- advanced by
// one += dt per step, as inside the kernels and in the reference loop, never k * dt -- and its slot of an n_slots-deep ring (0: no ring).
//   for (Chunks c{...}; c.k < c.n_steps; c.advance(ks))  with ks = c.len(), or less where the caller cuts a launch short
struct Chunks {
  int n_steps, per_launch;
  double t, dt;
  int slot, n_slots;
  int k = 0;
  int len() const { return n_steps - k < per_launch ? n_steps - k : per_launch; }
  void advance(int ks) {
    for (int j = 0; j < ks; ++j) t += dt;
    if (n_slots > 0) slot = (slot + ks) % n_slots;
    k += ks;
  }
};

// Run-time handle state -> template arguments.  Each helper calls a generic lambda with compile-time tags, so that a launch (its kernel
// name and argument list) is written once, in ordinary code, inside the lambda.  They instantiate exactly the branches listed here.
// with_flags(f, a, b, ...): f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...)
template <typename F> static void with_flags(F&& f) { f(); }
template <typename F, typename... Rest> static void with_flags(F&& f, bool b, Rest... rest) {
  if (b) with_flags([&](auto... r) { f(std::true_type{}, r...); }, rest...);
  else with_flags([&](auto... r) { f(std::false_type{}, r...); }, rest...);
}
// with_int<V0, V1, ...>(v, f): f(std::integral_constant<int, Vk>{}) for the Vk equal to v (the last one listed when none is)
template <int V, int... Vs, typename F> static void with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else with_int<Vs...>(v, f);
}
// dtype tag: T the compute type, S the storage type, COMP the compensated fp32 storage of MDS_F32C handles (fp32 buffers + state_lo)
template <typename T_, typename S_, bool COMP_ = false> struct DType {
  using T = T_;
  using S = S_;
  static constexpr bool COMP = COMP_;
};
// with_dtype: every dtype of mds.h, fp16 storage included (float arithmetic on half_t buffers)
template <typename F> static void with_dtype(int dtype, F&& f) {
  if (dtype == MDS_F32C) f(DType<float, float, true>{});
  else if (dtype == MDS_F32) f(DType<float, float>{});
  else if (dtype == MDS_F64) f(DType<double, double>{});
  else f(DType<float, half_t>{});
}
// with_dtype_no_half: the paths that are not built for fp16 storage (their entry points have refused MDS_F16 handles)
template <typename F> static void with_dtype_no_half(int dtype, F&& f) {
  if (dtype == MDS_F64) f(DType<double, double>{});
  else if (dtype == MDS_F32C) f(DType<float, float, true>{});
  else f(DType<float, float>{});
}

static inline dim3 grid_for(int n, int block) { return dim3((unsigned)((n + block - 1) / block)); }
static inline bool is_comp(const mds_handle* h) { return h->cfg.dtype == MDS_F32C; }
// the handle's Consts in both compute types (set-up path: after a change to cfg, the gains or the wind)
static void refill_consts(mds_handle* h) {
  fill_consts(h->cfg, h->gains, h->p32.c, h->wind);
  fill_consts(h->cfg, h->gains, h->p64.c, h->wind);
}

template <typename T> static void fill_lin_model(const double* A, const double* B, double u_eq0, LinModel<T>& M) {
  for (int r = 0; r < 12; ++r) {
    for (int k = 0; k < 12; ++k) M.A[r][k] = (T)A[r * 12 + k];
    for (int k = 0; k < 4; ++k) M.B[r][k] = (T)B[r * 4 + k];
  }
  M.ueq0 = (T)u_eq0;
}

template <typename T, typename S>
static void launch_compare_models(const Consts<T>& C, int count, const void* obs, const double* A, const double* B, double u_eq0, double dyn_m,
                                  const double* dyn_J, double dyn_g, void* xdot_lin, void* xdot_geo, void* x_lin, hipStream_t st) {
  LinModel<T> M;
  fill_lin_model<T>(A, B, u_eq0, M);
  k_compare_models<T, S><<<grid_for(count, kBlock), kBlock, 0, st>>>(C, M, count, (const S*)obs, (T)dyn_m, (T)dyn_J[0], (T)dyn_J[1], (T)dyn_J[2],
                                                                      (T)dyn_g, (S*)xdot_lin, (S*)xdot_geo, (S*)x_lin);
}
template <typename T, typename S>
static void launch_linear_xdot(const Consts<T>& C, int count, const void* x, const void* action, const double* A, const double* B, double u_eq0,
                               void* xdot, hipStream_t st) {
  LinModel<T> M;
  fill_lin_model<T>(A, B, u_eq0, M);
  k_linear_xdot<T, S><<<grid_for(count, 256), 256, 0, st>>>(C, M, count, (const S*)x, (const S*)action, (S*)xdot);
}

// set-up path: (re)write one gain struct to its device copy, synchronously
template <typename GF, typename GD> static int upload_gain(mds_handle* h, int slot, const GF& f32, const GD& f64) {
  if (int rc = h->mem.alloc(&h->gain_dev[slot], sizeof(f64))) return rc;
  if (h->cfg.dtype == MDS_F64) MDS_HIP(hipMemcpy(h->gain_dev[slot], &f64, sizeof(f64), hipMemcpyHostToDevice));
  else MDS_HIP(hipMemcpy(h->gain_dev[slot], &f32, sizeof(f32), hipMemcpyHostToDevice));
  return MDS_OK;
}

#if MDS_PART & 1
// the handle's randomisation as the kernels take it
template <typename T> static EpisodeRandomArgs<T> episode_random_args(const mds_handle* h) {
  const mds_episode_randomisation& p = h->ep_rand;
  EpisodeRandomArgs<T> a;
  fill_episode_random<T>(p.seed, (uint32_t)((unsigned long long)p.first_env * (unsigned long long)h->cfg.num_drones), h->ep_generation, p.pos,
                         p.rpy, p.vel, p.rate, a.set);
  a.rpy0 = h->init_pose + (size_t)3 * h->n;
  return a;
}
// what the two episode rollout entry points hand their kernels in compute type T, from the handle: the rule, the counters, the safety
// and the randomisation blocks (zeroed where the handle has none), the workgroup's share of envs and the grid
template <typename T> struct EpisodeLaunch {
  EpisodeRule<T> rule;
  EpisodeCounters<T> cnt;
  EpisodeSafetyArgs<T> safe;
  EpisodeRandomArgs<T> rnd;
  int D, epb;
  dim3 grid;
};
template <typename T> static EpisodeLaunch<T> episode_launch(const mds_handle* h) {
  const mds_episode_params& p = h->ep;
  EpisodeLaunch<T> a = {};
  fill_episode_rule<T>(p.max_steps, p.z_min, p.z_max, p.max_dist, p.max_tilt, p.max_speed, p.max_rate, p.reward_r0, p.term_penalty, a.rule);
  char* cb = (char*)h->ep_counters;
  const size_t sl = h->ep_slots * 8;
  a.cnt = {(int*)cb, (T*)(cb + sl), (int*)(cb + 2 * sl), (T*)(cb + 3 * sl), (int*)(cb + 4 * sl)};
  if (h->ep_safe) {
    fill_episode_safety<T>(h->ep_safety.safety_radius, h->ep_safety.zscale, h->ep_safety.n_obs, h->ep_obstacles, a.safe.set);
    a.safe.h_min_step = (T*)h->ep_hmin;
    a.safe.h_min_episode = (T*)((char*)h->ep_hmin + sl);
  }
  if (h->ep_random) a.rnd = episode_random_args<T>(h);
  a.D = h->cfg.num_drones;
  a.epb = episode_envs_per_block(a.D);
  a.grid = dim3((unsigned)((h->cfg.num_envs + a.epb - 1) / a.epb));
  return a;
}
// the handle's policy as the kernels take it
template <typename T> static EpisodePolicy<T> episode_policy_args(const mds_handle* h) {
  return {(const T*)h->ep_policy_w, h->ep_pol.n_hidden, h->ep_pol.activation, (T)h->ep_pol.rpm_base, (T)h->ep_pol.rpm_scale};
}
// the handle's action noise as the kernels take it
template <typename T> static PolicyNoise<T> episode_noise_args(const mds_handle* h) {
  const mds_episode_policy_noise& p = h->ep_noise_p;
  PolicyNoise<T> a;
  fill_policy_noise<T>(p.seed, (uint32_t)((unsigned long long)p.first_env * (unsigned long long)h->cfg.num_drones), h->ep_epoch, p.log_std, a);
  return a;
}
// the two dtypes the policy kernels are built for (mds_set_episode_policy has refused the others)
template <typename F> static void with_policy_dtype(int dtype, F&& f) {
  if (dtype == MDS_F64) f(DType<double, double>{});
  else f(DType<float, float>{});
}
#endif

extern "C" {

// (C linkage like everything in this block; not part of include/mds.h)
// helpers called across the two parts (defined once, in the part named)
// what step_nominal_lowlevel does besides nominal controller -> low level -> env.step
struct NominalStep {
  bool with_filter = false;       // the ECBF QP between the nominal controller and the low level
  EnvRange range = {0, -1, 0};    // the envs it steps (ne < 0: all of them)
  bool have_nominal = false;      // the previous step's low-level launch has left this step's u_hat / xdes in the scratch (its want_next)
  bool want_next = false;         // this step's low-level launch also computes the nominal input of the step at t_next (nominal 0 / 1 only)
  double t_next = 0.0;
};
int step_env_plain(mds_handle* h, const void* action, void* obs, hipStream_t st, int first_substep, void* home = nullptr);              // part 1
int step_env_ctrl(mds_handle* h, int ctrl, double t, const void* u_in, double thrust_offset, void* obs, void* act, hipStream_t st);     // part 1
int rollout_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs_last, void* stream, int ctrl, const char* who);       // part 1
int step_lqr(mds_handle* h, double t, void* obs, void* act, hipStream_t st);                                                            // part 2
int step_nominal_lowlevel(mds_handle* h, double t, void* obs, int32_t* status, void* action, hipStream_t st, const NominalStep& o = {}); // part 2

#if MDS_PART & 1
int mds_version(void) { return MDS_VERSION; }

const char* mds_strerror(int status) {
  switch (status) {
    case MDS_OK: return "ok";
    case MDS_EINVAL: return "invalid argument";
    case MDS_ENOMEM: return "out of device memory";
    case MDS_EHIP: return "HIP runtime error";
    case MDS_EALIGN: return "device pointer not 16-byte aligned";
    case MDS_ESTATE: return "call not valid in this handle state";
    case MDS_EUNSUPPORTED: return "unsupported combination";
    default: return "unknown status";
  }
}

const char* mds_last_error(void) { return g_err; }

int mds_default_config(int drone_model, mds_config* cfg) {
  if (!cfg || (drone_model != MDS_CF2X && drone_model != MDS_CF2P)) return fail(MDS_EINVAL, "mds_default_config");
  memset(cfg, 0, sizeof(*cfg));
  cfg->num_envs = 1;
  cfg->num_drones = 2;           // PIDEnv.py:29
  cfg->dtype = MDS_F32;
  cfg->physics = MDS_PHYSICS_DYN;
  cfg->integrator = MDS_INTEGRATOR_EULER;
  cfg->drone_model = drone_model;
  cfg->pyb_freq = 100;           // PIDEnv.py:24-25
  cfg->ctrl_freq = 100;
  cfg->M = 0.027;
  cfg->L = 0.0397;
  cfg->KF = 3.16e-10;
  cfg->KM = 7.94e-12;
  if (drone_model == MDS_CF2P) {
    cfg->J[0] = 2.3951e-5; cfg->J[1] = 2.3951e-5; cfg->J[2] = 3.2347e-5;
  } else {
    cfg->J[0] = 1.4e-5; cfg->J[1] = 1.4e-5; cfg->J[2] = 2.17e-5;
  }
  cfg->G = 9.8;
  cfg->thrust2weight = 2.25;
  cfg->drag_coeff[0] = 9.1785e-7; cfg->drag_coeff[1] = 9.1785e-7; cfg->drag_coeff[2] = 10.311e-7;
  return MDS_OK;
}

int mds_default_geometric_gains(mds_geometric_gains* g) {
  if (!g) return fail(MDS_EINVAL, "mds_default_geometric_gains");
  for (int k = 0; k < 3; ++k) {
    g->Kp[k] = 2.25; g->Kv[k] = 3.5; g->KR[k] = 125.0; g->Kw[k] = 10.0;   // control/geometric.py:14-17
  }
  g->g = 9.81;                                                             // :20
  g->max_tilt_angle = 40.0 * M_PI / 180.0;                                 // :23
  return MDS_OK;
}

int mds_create(const mds_config* cfg, mds_handle** out) {
  if (!cfg || !out) return fail(MDS_EINVAL, "mds_create: null argument");
  *out = nullptr;
  if (cfg->num_envs <= 0 || cfg->num_drones <= 0) return fail(MDS_EINVAL, "mds_create: num_envs/num_drones must be > 0");
  if ((long long)cfg->num_envs * cfg->num_drones > (1LL << 30)) return fail(MDS_EINVAL, "mds_create: too many drones");
  if (cfg->dtype < MDS_F32 || cfg->dtype > MDS_F32C) return fail(MDS_EINVAL, "mds_create: dtype");
  if (cfg->physics < MDS_PHYSICS_DYN || cfg->physics > MDS_PHYSICS_DYN_GND_DRAG_DW) return fail(MDS_EINVAL, "mds_create: physics");
  if (cfg->physics >= MDS_PHYSICS_DYN_GND && (cfg->integrator != MDS_INTEGRATOR_EULER || cfg->dtype == MDS_F16 || cfg->dtype == MDS_F32C))
    return fail(MDS_EINVAL, "mds_create: ground effect / downwash run with the explicit Euler integrator on f32 / f64 storage");
  if (cfg->integrator != MDS_INTEGRATOR_EULER && cfg->integrator != MDS_INTEGRATOR_RK4) return fail(MDS_EINVAL, "mds_create: integrator");
  if (cfg->drone_model != MDS_CF2X && cfg->drone_model != MDS_CF2P) return fail(MDS_EINVAL, "mds_create: drone_model");
  if (cfg->ctrl_freq <= 0 || cfg->pyb_freq <= 0 || cfg->pyb_freq % cfg->ctrl_freq != 0)
    return fail(MDS_EINVAL, "mds_create: pyb_freq must be a positive multiple of ctrl_freq");
  if (!(cfg->M > 0) || !(cfg->KF > 0) || !(cfg->KM > 0) || !(cfg->L > 0) || !(cfg->J[0] > 0) || !(cfg->J[1] > 0) || !(cfg->J[2] > 0))
    return fail(MDS_EINVAL, "mds_create: non-positive drone constant");
  DevGuard dev_guard__(cfg->device);        // the caller's current device is restored on return
  if (dev_guard__.err != hipSuccess) return fail_hip(dev_guard__.err, "mds_create: hipSetDevice(cfg->device)");
  mds_handle* h = new (std::nothrow) mds_handle(kHipAllocator);
  if (!h) return fail(MDS_ENOMEM, "mds_create: host allocation");
  h->cfg = *cfg;
  mds_default_geometric_gains(&h->gains);
  h->n = cfg->num_envs * cfg->num_drones;
  h->ld = ((size_t)h->n + 255) / 256 * 256;
  refill_consts(h);
  const size_t es = elem_size(cfg->dtype), cs = comp_size(cfg->dtype);
  h->envfx = cfg->physics >= MDS_PHYSICS_DYN_GND;
  fill_envfx(h->cfg, h->p32.fx);
  fill_envfx(h->cfg, h->p64.fx);
  h->track_rpm = cfg->track_last_rpm != 0 || cfg->physics == MDS_PHYSICS_DYN_DRAG || cfg->physics == MDS_PHYSICS_DYN_GND_DRAG_DW;
  {
    mds_dslpid_gains dg;
    mds_default_dslpid_gains(&dg);
    mds_set_dslpid_gains(h, &dg);
  }
  std::vector<DevMem::Want> bufs = {{&h->state, 13 * h->ld * es, true},
                                    {&h->origin, 3 * h->ld * cs, true},
                                    {&h->last_rpm, 4 * h->ld * cs, true},
                                    {&h->lem, 7 * h->ld * cs, true},
                                    {&h->scratch, (size_t)h->n * 20 * sizeof(double), true},      // (zeros: the identity attitude below)
                                    {&h->ll, 6 * h->ld * cs, true},
                                    {&h->pid, 9 * h->ld * cs, true}};
  if (is_comp(h)) bufs.push_back({&h->state_lo, 4 * h->ld * es, true});
  if (h->envfx) {
    bufs.push_back({&h->state_alt, 13 * h->ld * es, true});
    bufs.push_back({&h->act_scratch, (size_t)h->n * 4 * es});
  }
  int rc = h->mem.alloc_all(bufs);
  // identity attitude
  if (rc == MDS_OK) {
    with_dtype(h->cfg.dtype, [&](auto DT) {
      using T = typename decltype(DT)::T;
      using S = typename decltype(DT)::S;
      k_reset<T, S><<<grid_for(h->n, 256), 256, 0, 0>>>(h->n, h->ld, h->scratch, h->scratch + (size_t)3 * h->n, (const T*)h->origin, (S*)h->state,
                                                         (T*)h->last_rpm, 0, (S*)h->state_lo);
    });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = fail_hip(e, "mds_create: identity attitude");
  }
  // shards large enough for the auto policy of the two-chain rollouts get their streams and events now (smallest auto
  // threshold: the CBF loop, 2^16 drones); smaller ones only if mds_set_rollout_streams(h, 2) asks for them
  if (rc == MDS_OK && (size_t)h->n >= kSplitMinDrones / 4) rc = split_streams_ready(h);
  if (rc != MDS_OK) {            // every failure after `new`: the handle and whatever it owns by now go through mds_destroy
    mds_destroy(h);
    return rc;
  }
  *out = h;
  return MDS_OK;
}

int mds_destroy(mds_handle* h) {
  if (!h) return MDS_OK;
  MDS_DEV(h);
  h->mem.release_all();
  if (h->split_st) (void)hipStreamDestroy(h->split_st);
  for (int k = 0; k < 2; ++k)
    if (h->split_ev[k]) (void)hipEventDestroy(h->split_ev[k]);
  delete h;
  return MDS_OK;
}

int mds_get_derived(const mds_handle* h, double out[8]) {
  if (!h || !out) return fail(MDS_EINVAL, "mds_get_derived");
  const mds_config& c = h->cfg;
  const double grav = c.G * c.M;
  const double max_rpm = sqrt(c.thrust2weight * grav / (4 * c.KF));
  out[0] = grav;
  out[1] = sqrt(grav / (4 * c.KF));
  out[2] = max_rpm;
  out[3] = 4 * c.KF * max_rpm * max_rpm;
  out[4] = c.drone_model == MDS_CF2X ? (2 * c.L * c.KF * max_rpm * max_rpm) / sqrt(2.0) : c.L * c.KF * max_rpm * max_rpm;
  out[5] = 2 * c.KM * max_rpm * max_rpm;
  out[6] = 1.0 / c.ctrl_freq;
  out[7] = 1.0 / c.pyb_freq;
  return MDS_OK;
}

// drones [i0, i1) back to the poses of the last mds_reset (zero velocities, zero RPM echo); enqueue only
static int launch_reset_range(mds_handle* h, hipStream_t st, size_t i0, size_t i1) {
  const double* xyz = h->init_pose;
  const double* rpy = h->init_pose + (size_t)3 * h->n;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_reset<T, S><<<grid_for(i1 - i0, 256), 256, 0, st>>>((int)i1, h->ld, xyz, rpy, (const T*)h->origin, (S*)h->state, (T*)h->last_rpm, (int)i0,
                                                           (S*)h->state_lo);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

// Per-env episodes, set-up side: the reset image is what mds_reset_async would write -- k_reset itself, into the library's second state
// buffer -- and the local-frame targets are formed against the current origin; both are rebuilt whenever the poses (mds_reset) or the
// origin (mds_set_origin and the trajectory uploads that call it) change.  Enqueue only.
static int episode_build_image(mds_handle* h, hipStream_t st) {
  const double* xyz = h->init_pose;
  const double* rpy = h->init_pose + (size_t)3 * h->n;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    // (k_reset also zeroes four RPM planes: the target buffer has room for them, and the targets are written after it, in stream order)
    k_reset<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(h->n, h->ld, xyz, rpy, (const T*)h->origin, (S*)h->ep_image, (T*)h->ep_target, 0, (S*)nullptr);
    k_episode_targets<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(h->n, h->ld, h->ep_target_world, (const T*)h->origin, (const S*)h->ep_image,
                                                                   (T*)h->ep_target);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}
// [first, first + count) of the two h_min arrays (0: h_min_step, 1: h_min_episode) back to +inf.  Enqueue only.
static int episode_hmin_clear(mds_handle* h, hipStream_t st, void* block, int first, int count) {
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T;
    const int m = (int)(h->ep_slots * count * (8 / sizeof(T)));          // the arrays are 8-byte slots whatever T is: their whole extent
    k_episode_fill_inf<T><<<grid_for(m, 256), 256, 0, st>>>(m, (T*)((char*)block + (size_t)first * h->ep_slots * 8));
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}
// the running episode of every env starts anew (length, return, smallest h); the statistics of the completed ones stay
static int episode_restart(mds_handle* h, hipStream_t st) {
  MDS_HIP(hipMemsetAsync(h->ep_counters, 0, 2 * h->ep_slots * 8, st));
  if (h->ep_hmin)
    if (int rc = episode_hmin_clear(h, st, h->ep_hmin, 1, 1)) return rc;
  ++h->ep_epoch;                       // (mds_policy_noise.hpp: the same count and length must not replay the same noise; a failed restart moves nothing)
  return MDS_OK;
}

int mds_reset(mds_handle* h, const double* xyz, const double* rpy, void* stream) {
  MDS_DEV(h);
  if (!h || !xyz || !rpy) return fail(MDS_EINVAL, "mds_reset: null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = (size_t)h->n * 3 * sizeof(double);
  if (int rc = h->mem.alloc(&h->init_pose, 2 * nb)) return rc;
  MDS_HIP(hipMemcpyAsync(h->init_pose, xyz, nb, hipMemcpyHostToDevice, st));
  MDS_HIP(hipMemcpyAsync(h->init_pose + (size_t)3 * h->n, rpy, nb, hipMemcpyHostToDevice, st));
  if (int rc = launch_reset_range(h, st, 0, h->n)) return rc;
  MDS_HIP(hipMemsetAsync(h->ll, 0, 6 * h->ld * comp_size(h->cfg.dtype), st));
  MDS_HIP(hipMemsetAsync(h->pid, 0, 9 * h->ld * comp_size(h->cfg.dtype), st));
  h->rpm_stale = false;
  if (h->ep_on) {                      // new poses: a new reset image, and every env's running episode starts anew
    if (int rc = episode_build_image(h, st)) return rc;
    if (int rc = episode_restart(h, st)) return rc;
  }
  MDS_HIP(hipStreamSynchronize(st));   // host buffers may be reused by the caller
  return MDS_OK;
}

int mds_reset_async(mds_handle* h, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_reset_async: null handle");
  if (!h->init_pose) return fail(MDS_ESTATE, "mds_reset_async: no mds_reset yet");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_reset_range(h, st, 0, h->n)) return rc;
  MDS_HIP(hipMemsetAsync(h->ll, 0, 6 * h->ld * comp_size(h->cfg.dtype), st));
  MDS_HIP(hipMemsetAsync(h->pid, 0, 9 * h->ld * comp_size(h->cfg.dtype), st));
  h->rpm_stale = false;
  if (h->ep_on)
    if (int rc = episode_restart(h, st)) return rc;
  return MDS_OK;
}

int mds_state_ptrs(mds_handle* h, void* comp_dev[13], size_t stride_elems[13], void* origin_dev[3]) {
  MDS_DEV(h);
  if (!h || !comp_dev || !stride_elems) return fail(MDS_EINVAL, "mds_state_ptrs: null argument");
  const size_t es = elem_size(h->cfg.dtype), cs = comp_size(h->cfg.dtype);
  for (int k = 0; k < 13; ++k) {
    comp_dev[k] = (char*)h->state + sidx(k, 0, h->ld) * es;
    stride_elems[k] = k < 12 ? 4 : 1;
  }
  if (origin_dev)
    for (int k = 0; k < 3; ++k) origin_dev[k] = (char*)h->origin + (size_t)k * h->ld * cs;
  return MDS_OK;
}

int mds_get_state(mds_handle* h, double* out, void* stream) {
  MDS_DEV(h);
  if (!h || !out) return fail(MDS_EINVAL, "mds_get_state: null argument");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_get_state<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(h->n, h->ld, (const S*)h->state, (const T*)h->origin, h->scratch, (const S*)h->state_lo);
  });
  MDS_HIP(hipGetLastError());
  MDS_HIP(hipMemcpyAsync(out, h->scratch, (size_t)h->n * 13 * sizeof(double), hipMemcpyDeviceToHost, st));
  MDS_HIP(hipStreamSynchronize(st));
  return MDS_OK;
}

int mds_set_state(mds_handle* h, const double* in, void* stream) {
  MDS_DEV(h);
  if (!h || !in) return fail(MDS_EINVAL, "mds_set_state: null argument");
  hipStream_t st = (hipStream_t)stream;
  MDS_HIP(hipMemcpyAsync(h->scratch, in, (size_t)h->n * 13 * sizeof(double), hipMemcpyHostToDevice, st));
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_set_state<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(h->n, h->ld, h->scratch, (const T*)h->origin, (S*)h->state, (S*)h->state_lo);
  });
  MDS_HIP(hipGetLastError());
  MDS_HIP(hipStreamSynchronize(st));
  return MDS_OK;
}

int mds_set_origin(mds_handle* h, const double* origin, void* stream) {
  MDS_DEV(h);
  if (!h || !origin) return fail(MDS_EINVAL, "mds_set_origin: null argument");
  hipStream_t st = (hipStream_t)stream;
  MDS_HIP(hipMemcpyAsync(h->scratch, origin, (size_t)h->n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_set_origin<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(h->n, h->ld, h->scratch, (T*)h->origin, (S*)h->state, (S*)h->state_lo);
  });
  MDS_HIP(hipGetLastError());
  if (h->ep_on)                        // the reset image and the targets are local-frame values
    if (int rc = episode_build_image(h, st)) return rc;
  MDS_HIP(hipStreamSynchronize(st));
  return MDS_OK;
}

int mds_get_obs(mds_handle* h, void* obs, void* stream) {
  MDS_DEV(h);
  if (!h || !obs) return fail(MDS_EINVAL, "mds_get_obs: null argument");
  if (!aligned16(obs)) return fail(MDS_EALIGN, "mds_get_obs: obs_dev");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_get_obs<T, S><<<grid_for(h->n, kBlock), kBlock, 0, st>>>(h->n, h->ld, (const S*)h->state, (const T*)h->origin,
                                                                (const T*)(h->rpm_stale ? nullptr : h->last_rpm), (S*)obs);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

// Unused dynamic LDS of a half-shard launch in a two-chain rollout (step_geometric says why).  stages_rows: the kernel has its
// static LDS block for the observation rows (or the segment tables), else only its 16-byte minimum.
static size_t split_lds_pad(const mds_handle* h, bool stages_rows) {
  const size_t static_lds = stages_rows ? (size_t)kBlock * kObsDim * elem_size(h->cfg.dtype) : 16;
  return static_lds < kSplitLds ? kSplitLds - static_lds : 0;
}

// One env.step of the batches ch covers: k_step; half-shard launches of a two-chain rollout are padded to 32 KB LDS like the fused
// step's (step_geometric).  Ground effect / downwash handles (always one chain): one launch per substep, step_env_plain.
// Like every step_* function below it only enqueues; the caller checks hipGetLastError once after its last launch.
static int step_plain(mds_handle* h, const void* action, void* obs, const Chain& ch) {
  hipStream_t st = ch.st;
  if (h->envfx) return step_env_plain(h, action, obs, st, 0);
  const unsigned batch0 = ch.i0, nb = ch.n;
  const dim3 grid(nb ? nb : (unsigned)((h->n + kBlock - 1) / kBlock));
  const size_t pad = nb ? split_lds_pad(h, obs != nullptr) : 0;
  with_flags([&](auto HAS_OBS, auto RK4, auto DRAG) {
    with_dtype(h->cfg.dtype, [&](auto DT) {
      using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
      k_step<T, S, HAS_OBS(), RK4(), DRAG(), DT.COMP><<<grid, kBlock, pad, st>>>(params<T>(h).c, h->n, h->ld, (S*)h->state, (const T*)h->origin,
                                                                                  (T*)rpm_track(h), (const S*)action, (S*)obs, (int)batch0,
                                                                                  (S*)h->state_lo);
    });
  }, obs != nullptr, h->cfg.integrator == MDS_INTEGRATOR_RK4, has_drag(h));
  return MDS_OK;
}

// [UPSTREAM] BaseAviary.step under ground effect / downwash: one launch per physics substep on the double-buffered state
// (k_step_env).  first_substep: substeps [first_substep, K) are run (a controller kernel has already done substep 0 and left its
// action in `action`).
// Stream capture and the double-buffered state.  Every substep reads one buffer, writes the other and flips the handle's pointers on
// the host; a captured call bakes the pointers of the moment into its graph, so a call with an odd number of substeps would replay
// A -> B every time and never advance.  Under capture such a call ends with a copy of the state back into the buffer it started
// from (`home`) and leaves the handle pointing there: every replay then starts and ends in the same buffer.  Eager calls flip only.
static bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
static int envfx_return_home(mds_handle* h, void* home, hipStream_t st) {
  if (h->state == home || !stream_is_capturing(st)) return MDS_OK;
  MDS_HIP(hipMemcpyAsync(home, h->state, 13 * h->ld * elem_size(h->cfg.dtype), hipMemcpyDeviceToDevice, st));
  h->state_alt = h->state;
  h->state = home;
  return MDS_OK;
}

int step_env_plain(mds_handle* h, const void* action, void* obs, hipStream_t st, int first_substep, void* home) {
  const dim3 grid = grid_for(h->n, kBlock);
  const int K = h->cfg.pyb_freq / h->cfg.ctrl_freq, D = h->cfg.num_drones;
  void* rpm = rpm_track(h);
  if (!home) home = h->state;
  for (int k = first_substep; k < K; ++k) {
    void* ob = k == K - 1 ? obs : nullptr;
    with_dtype_no_half(h->cfg.dtype, [&](auto DT) {        // ground effect / downwash: f32 / f64 storage only (mds_create)
      using T = typename decltype(DT)::T;
      with_flags([&](auto DRAG) {
        k_step_env<T, T, DRAG()><<<grid, kBlock, 0, st>>>(params<T>(h).c, params<T>(h).fx, h->n, h->ld, D, (const T*)h->state, (T*)h->state_alt,
                                                          (const T*)h->origin, (T*)rpm, (const T*)action, (T*)ob, k > 0, k == K - 1);
      }, has_drag(h));
    });
    void* t = h->state; h->state = h->state_alt; h->state_alt = t;
  }
  MDS_HIP(hipGetLastError());
  return envfx_return_home(h, home, st);
}

// One control step of a controller path under ground effect / downwash: k_step_ctrl_env (trajectory sample or given input ->
// controller -> first substep), then the remaining substeps through k_step_env with the action it left in act_scratch.
// ctrl 0 GeometricControl, 1 LQRController (12-state), 2 ThrustOmega low level on u_in, 3 YankOmega low level on u_in.
int step_env_ctrl(mds_handle* h, int ctrl, double t, const void* u_in, double thrust_offset, void* obs, void* act, hipStream_t st) {
  const dim3 grid = grid_for(h->n, kBlock);
  const int K = h->cfg.pyb_freq / h->cfg.ctrl_freq, D = h->cfg.num_drones;
  void* rpm = rpm_track(h);
  void* abuf = K > 1 ? h->act_scratch : nullptr;
  const void* gain = ctrl == 1 ? h->gain_dev[0] : nullptr;
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {          // ground effect / downwash: f32 / f64 storage only (mds_create)
    using T = typename decltype(DT)::T;
    with_int<0, 1, 2, 3>(ctrl, [&](auto CTRL) {
      with_flags([&](auto DRAG) {
        k_step_ctrl_env<T, T, DRAG(), CTRL()><<<grid, kBlock, 0, st>>>(params<T>(h).c, params<T>(h).fx, gain, h->n, h->ld, D, t, h->traj_mode,
                                                                       (const T*)h->state, (T*)h->state_alt, (const T*)h->origin, (const T*)h->lem,
                                                                       SegTable{h->segs, h->nseg_total}, h->tinfo, (T*)rpm, (T*)h->ll, (const T*)u_in,
                                                                       (T)(1.0 / h->cfg.ctrl_freq), (T)thrust_offset, (T*)abuf, (T*)obs, (T*)act, K == 1);
      }, has_drag(h));
    });
  });
  MDS_HIP(hipGetLastError());
  void* home = h->state;
  void* tmp = h->state; h->state = h->state_alt; h->state_alt = tmp;
  if (K > 1) return step_env_plain(h, h->act_scratch, obs, st, 1, home);
  return envfx_return_home(h, home, st);
}

int mds_step(mds_handle* h, const void* action, void* obs, void* stream) {
  MDS_DEV(h);
  if (!h || !action) return fail(MDS_EINVAL, "mds_step: null argument");
  if (!aligned16(action) || !aligned16(obs)) return fail(MDS_EALIGN, "mds_step: action_dev/obs_dev");
  if (int rc = step_plain(h, action, obs, Chain{(hipStream_t)stream, 0, 0})) return rc;
  return check_launches();
}

// The phase table (mds_kernels.hip, TAB): kPhaseTabRows control steps of 64 (sin, cos) pairs, 1 MB in fp32, filled by
// k_lemniscate_phase_table on the stream of the launch that needs rows (phase_table_rows has the policy: a launch that does not
// continue the last one fills its own rows, a continuing flight doubles its fills up to the whole table, which then serves 40
// launches of 50 steps).  The whole-rollout loop has the table form where its step is the leanest: fp32
// arithmetic and storage, Euler, no drag, GeometricControl (launch_rollout_kernel).  RK4, drag, compensated and fp16 storage and float64
// compute the phase in the kernel: the same bits either way, so which launches read the table is the library's choice.
// Where the amplitudes repeat as well (lemniscate_desired_periodic) the block is 4 MB and its rows hold the eight values the controller
// reads of the desired state (LemDesired8) instead of the pair: same fills, same bookkeeping, k_rollout_geometric_y0d.
constexpr int kPhaseTabRows = 2048;
static bool phase_table_built(const mds_handle* h) {
  return h->cfg.dtype == MDS_F32 && h->cfg.integrator != MDS_INTEGRATOR_RK4 && !has_drag(h) && !h->envfx;
}
// (wide: rows of 64 x 8 values, the desired-state table; a block of that size serves the narrow rows too)
static size_t phase_table_bytes(const mds_handle* h, bool wide) { return (size_t)kPhaseTabRows * kPhaseLanes * (wide ? 8 : 2) * comp_size(h->cfg.dtype); }

int mds_set_lemniscate(mds_handle* h, const double* params, void* stream) {
  MDS_DEV(h);
  if (!h || !params) return fail(MDS_EINVAL, "mds_set_lemniscate: null argument");
  hipStream_t st = (hipStream_t)stream;
  const int n = h->n;
  // re-base the local frame onto the trajectory centres (host gathers them from params)
  double* centres = new (std::nothrow) double[(size_t)n * 3];
  if (!centres) return fail(MDS_ENOMEM, "mds_set_lemniscate: host allocation");
  bool yaw_free = true;          // decided per upload, for the whole handle: every kernel that serves it then takes the same form
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) centres[(size_t)3 * i + k] = params[(size_t)7 * i + 2 + k];
    yaw_free = yaw_free && params[(size_t)7 * i + 5] == 0.0;
  }
  // the lanes of every wave share their phases (mds_traj_phase_periodic): the first upload of that kind on a handle whose whole-rollout
  // loop has the table form (phase_table_built) gets the table's block -- before anything of the handle changes: out of memory leaves it as it was
  // An upload whose amplitudes repeat as well (mds_traj_desired_periodic) gets the block of the wide rows, in place of a narrow one
  // an earlier upload may have left: the new block first, then the old one freed.
  const bool phase_periodic = lemniscate_phase_periodic(params, n), desired_periodic = lemniscate_desired_periodic(params, n);
  if (yaw_free && phase_periodic && phase_table_built(h)) {
    const size_t want = phase_table_bytes(h, desired_periodic);
    if (h->phase_tab_bytes < want) {
      const int arc = h->phase_tab ? h->mem.replace(&h->phase_tab, want, [](void*) { return 0; }) : h->mem.alloc(&h->phase_tab, want);
      if (arc) {
        delete[] centres;
        return arc;
      }
      h->phase_tab_bytes = want;
      h->phase_tab_filled = false;
    }
  }
  int rc = mds_set_origin(h, centres, stream);
  delete[] centres;
  if (rc != MDS_OK) return rc;
  MDS_HIP(hipMemcpyAsync(h->scratch, params, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, st));
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T;
    k_set_planes<T><<<grid_for(n, 256), 256, 0, st>>>(n, h->ld, 7, h->scratch, (T*)h->lem);
  });
  MDS_HIP(hipGetLastError());
  MDS_HIP(hipStreamSynchronize(st));
  h->has_traj = true;
  h->traj_mode = 1;
  h->traj_yaw_free = yaw_free;
  h->traj_phase_periodic = phase_periodic;
  h->traj_desired_periodic = desired_periodic;
  h->phase_tab_filled = false;           // new phases: the rows are refilled by the next launch that reads them
  return MDS_OK;
}

int mds_traj_yaw_free(mds_handle* h) { return h && h->traj_yaw_free ? 1 : 0; }
int mds_traj_phase_periodic(mds_handle* h) { return h && h->traj_phase_periodic ? 1 : 0; }
int mds_traj_desired_periodic(mds_handle* h) { return h && h->traj_desired_periodic ? 1 : 0; }

int mds_set_traj_specialisation(mds_handle* h, int on) {
  if (!h) return fail(MDS_EINVAL, "mds_set_traj_specialisation: null handle");
  h->traj_spec = on != 0;
  return MDS_OK;
}

int mds_set_traj_phase_table(mds_handle* h, int on) {
  if (!h) return fail(MDS_EINVAL, "mds_set_traj_phase_table: null handle");
  h->phase_tab_on = on != 0;
  return MDS_OK;
}

int mds_set_traj_desired_table(mds_handle* h, int on) {
  if (!h) return fail(MDS_EINVAL, "mds_set_traj_desired_table: null handle");
  h->desired_tab_on = on != 0;
  return MDS_OK;
}

int mds_get_last_rollout_phase_table(mds_handle* h) { return h ? h->last_rollout_phase_table : 0; }
int mds_get_last_rollout_desired_table(mds_handle* h) { return h ? h->last_rollout_desired_table : 0; }

// the fused GeometricControl step and the whole-rollout kernel take the yaw-free form together (both launch forms, every dtype)
static bool use_yaw_free(const mds_handle* h) { return h->traj_mode == 1 && h->traj_yaw_free && h->traj_spec; }

int mds_set_trajectory_segments(mds_handle* h, const double* segs, const int32_t* offsets, const int32_t* compound,
                                const double* anchor, int32_t total, void* stream) {
  MDS_DEV(h);
  if (!h || !segs || !offsets || !compound || !anchor) return fail(MDS_EINVAL, "mds_set_trajectory_segments: null argument");
  const int n = h->n;
  // validation, de-duplication and the field-major / piece-major image: host code of its own (csrc/mds_traj_image.hpp)
  std::vector<int> ti;
  std::vector<double> fm;
  int nu = 0;
  const char* why = "";
  const int brc = build_traj_image(segs, offsets, compound, n, total, fm, ti, nu, &why);
  if (brc != MDS_OK) return fail(brc, why);
  if (int rc = h->mem.alloc(&h->tinfo, sizeof(int) * 3 * n)) return rc;
  // the new segment table is complete on the device before the one in use is given up: whatever fails on the way, the previous
  // upload (tables, nseg_total, has_traj, traj_mode, traj_yaw_free) keeps flying
  const int rc = h->mem.replace(&h->segs, sizeof(double) * fm.size(), [&](void* new_segs) -> int {
    MDS_HIP(hipMemcpy(new_segs, fm.data(), sizeof(double) * fm.size(), hipMemcpyHostToDevice));
    if (int orc = mds_set_origin(h, anchor, stream)) return orc;
    MDS_HIP(hipMemcpy(h->tinfo, ti.data(), sizeof(int) * 3 * n, hipMemcpyHostToDevice));
    return MDS_OK;
  });
  if (rc != MDS_OK) return rc;
  h->nseg_total = nu;
  h->has_traj = true;
  h->traj_mode = 2;
  h->traj_yaw_free = false;
  h->traj_phase_periodic = false;
  h->traj_desired_periodic = false;
  return MDS_OK;
}

int mds_traj_eval(mds_handle* h, double t, void* des, void* stream) {
  MDS_DEV(h);
  if (!h || !des) return fail(MDS_EINVAL, "mds_traj_eval: null argument");
  if (h->traj_mode == 1) return mds_lemniscate_eval(h, t, des, stream);
  if (h->traj_mode != 2) return fail(MDS_ESTATE, "mds_traj_eval: no trajectories set");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using S = typename decltype(DT)::S;
    k_traj_eval<S><<<grid_for(h->n, 256), 256, 0, st>>>(h->n, t, SegTable{h->segs, h->nseg_total}, h->tinfo, (S*)des);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_set_geometric_gains(mds_handle* h, const mds_geometric_gains* g) {
  if (!h || !g) return fail(MDS_EINVAL, "mds_set_geometric_gains: null argument");
  if (!(g->max_tilt_angle > 0) || !(g->max_tilt_angle < M_PI / 2)) return fail(MDS_EINVAL, "mds_set_geometric_gains: max_tilt_angle");
  h->gains = *g;
  refill_consts(h);
  return MDS_OK;
}

int mds_set_wind(mds_handle* h, const double force_world[3]) {
  if (!h || !force_world) return fail(MDS_EINVAL, "mds_set_wind: null argument");
  for (int k = 0; k < 3; ++k) h->wind[k] = force_world[k];
  refill_consts(h);
  return MDS_OK;
}

// One fused control step (trajectory sample -> GeometricControl -> env.step) of the 256-drone batches ch covers; ground effect /
// downwash handles (always one chain): the controller with the first substep, then one launch per remaining substep (step_env_ctrl).
static int step_geometric(mds_handle* h, double t, void* obs, void* act, const Chain& ch) {
  hipStream_t st = ch.st;
  if (h->envfx) return step_env_ctrl(h, 0, t, nullptr, 0.0, obs, act, st);
  const unsigned batch0 = ch.i0, nb = ch.n;
  const unsigned nbatch = nb ? nb : (unsigned)((h->n + kBlock - 1) / kBlock);
  // A chain that covers part of the shard (n != 0: a half, in a two-chain rollout) launches with unused dynamic LDS, so that its
  // workgroups occupy kSplitLds = 32 KB each, static block included (split_lds_pad): 5 workgroups per CU instead of 8.  A half then
  // no longer fits the chip next to the other chain's half, so its workgroups enter as the other chain's retire and the two chains
  // interleave from the first step on (C3: 15.6 -> 15.0 us per step over 20 000 steps, 16.5 -> 15.8 over 2000; on one stream the
  // same padding costs 4 %, so whole-shard launches do not get it).
  const size_t pad = nb ? split_lds_pad(h, h->traj_mode == 2 || obs) : 0;
  const dim3 grid(nbatch);
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  if (h->traj_mode == 2) {      // general trajectories: segment tables
    with_flags([&](auto RK4, auto DRAG) {
      with_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
        k_step_traj<T, S, RK4(), DRAG(), DT.COMP><<<grid, kBlock, pad, st>>>(params<T>(h).c, h->n, h->ld, t, (S*)h->state, (const T*)h->origin,
                                                                             SegTable{h->segs, h->nseg_total}, h->tinfo, (T*)rpm_track(h), (S*)obs,
                                                                             (S*)act, (int)batch0, (S*)h->state_lo);
      });
    }, rk4, drag);
    return MDS_OK;
  }
  with_flags([&](auto Y0, auto HAS_OBS, auto HAS_ACT, auto RK4, auto DRAG) {
    with_dtype(h->cfg.dtype, [&](auto DT) {
      using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
      auto* const k = Y0() ? &k_step_geometric_y0<T, S, HAS_OBS(), HAS_ACT(), RK4(), DRAG(), DT.COMP>
                           : &k_step_geometric<T, S, HAS_OBS(), HAS_ACT(), RK4(), DRAG(), DT.COMP>;
      k<<<grid, kBlock, pad, st>>>(params<T>(h).c, h->n, h->ld, t, (S*)h->state, (const T*)h->lem, (T*)rpm_track(h), (S*)obs, (S*)act, (int)batch0,
                                   (S*)h->state_lo);
    });
  }, use_yaw_free(h), obs != nullptr, act != nullptr, rk4, drag);
  return MDS_OK;
}

int mds_step_geometric(mds_handle* h, double t, void* obs, void* act, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_step_geometric: null handle");
  if (!h->has_traj) return fail(MDS_ESTATE, "mds_step_geometric: call mds_set_lemniscate first");
  if (!aligned16(obs) || !aligned16(act)) return fail(MDS_EALIGN, "mds_step_geometric: obs_dev/action_dev");
  if (int rc = step_geometric(h, t, obs, act, Chain{(hipStream_t)stream, 0, 0})) return rc;
  return check_launches();
}

// The table rows of a launch of n_steps control steps from t0 (use_phase_table holds), filled on st where they are not there yet.
// A launch that starts at the time the last one ended at, to the bit, reads on behind it; when it would run past the rows that are
// filled, the table is filled from its first step, twice as many rows as the time before up to all 2048 (a flight of many launches: 40
// of 50 steps per fill).  A launch at any other time -- a caller that passes k * dt, the first call of a flight -- fills its own n_steps
// rows only: a fill costs its longest chain of dependent additions, and a short call must not pay for 2048 steps it may never fly.
// (fp32: the handles phase_table_built admits)
// wide: rows of the desired-state table (use_desired_table holds); rows of the other layout count as not filled.
static const float* phase_table_rows(mds_handle* h, double t0, double dt, int n_steps, bool wide, hipStream_t st) {
  using T = float;
  const bool continues = h->phase_tab_filled && h->phase_tab_wide == wide && memcmp(&t0, &h->phase_tab_t, sizeof(double)) == 0;
  if (!continues || h->phase_tab_row + n_steps > h->phase_tab_rows) {
    const int rows = continues ? std::min(kPhaseTabRows, std::max(2 * h->phase_tab_rows, n_steps)) : n_steps;
    auto* const fill = wide ? &k_lemniscate_phase_table<T, true> : &k_lemniscate_phase_table<T, false>;
    fill<<<grid_for((size_t)rows * kPhaseLanes, 256), 256, 0, st>>>(h->n, h->ld, t0, dt, rows, (const T*)h->lem, (T*)h->phase_tab);
    h->phase_tab_filled = true;
    h->phase_tab_wide = wide;
    h->phase_tab_rows = rows;
    h->phase_tab_row = 0;
  }
  const T* first = (const T*)h->phase_tab + (size_t)h->phase_tab_row * kPhaseLanes * (wide ? 8 : 2);
  h->phase_tab_row += n_steps;
  for (int k = 0; k < n_steps; ++k) t0 += dt;        // (as Chunks::advance and the kernel's loop)
  h->phase_tab_t = t0;
  return first;
}
// A launch that is being captured into a graph does not read the table: what the rows hold is bookkeeping of the host, true at the
// moment of an eager enqueue.  A captured launch would bake a pointer to rows that later calls and uploads overwrite before a replay,
// and a captured fill would mark rows as filled that no kernel has written yet.  Such a launch computes the phase in the kernel (the
// same bits), from the t0 and the planes baked into it, and leaves the bookkeeping as it found it.
static bool use_phase_table(const mds_handle* h, int n_steps, hipStream_t st) {
  return use_yaw_free(h) && h->traj_phase_periodic && h->phase_tab_on && h->phase_tab && n_steps >= 1 && n_steps <= kPhaseTabRows &&
         !stream_is_capturing(st);
}
// ... and the wide rows where the amplitudes repeat too, the block has their size and mds_set_traj_desired_table has not switched them off
static bool use_desired_table(const mds_handle* h, int n_steps, hipStream_t st) {
  return use_phase_table(h, n_steps, st) && h->traj_desired_periodic && h->desired_tab_on && h->phase_tab_bytes >= phase_table_bytes(h, true);
}

// One launch of the whole-rollout kernel: n_steps control steps with the state in registers.  ctrl: 0 GeometricControl, 1 LQRController
// (12-state), 2 LQROmegaController + ThrustOmega, 3 LQRYankOmegaController + YankOmega (Lemniscate trajectories only, no fp16 storage:
// rollout_fused has refused the rest).  Step k's observation goes to obs_log + k * log_stride
// elements (log_stride = n * 20: a [n_steps, n, 20] log; 0: every step overwrites the same [n, 20] buffer, what a step-by-step loop with one
// observation buffer does); obs_last (or NULL) receives the last step's.
static void launch_rollout_kernel(mds_handle* h, int ctrl, double t0, int n_steps, void* obs_log, size_t log_stride, void* obs_last, hipStream_t st) {
  const dim3 grid = grid_for(h->n, kBlock);
  const double dt = 1.0 / h->cfg.ctrl_freq;
  const int omode = obs_log == nullptr ? kObsLast : log_stride == 0 ? kObsInPlace : kObsLog;
  h->last_rollout_phase_table = h->last_rollout_desired_table = 0;
  auto launch = [&](auto DT, auto CTRL) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    constexpr int COMP = DT.COMP ? 1 : 0;
    // the gain (up to 48 values) is read from its device copy: passing it by value would not fit beside Consts in SGPRs
    const void* gain = nullptr;
    if constexpr (CTRL() >= 1) gain = h->gain_dev[CTRL() - 1];
    with_flags([&](auto RK4, auto DRAG) {
      auto roll = [&](auto OBS) {
        if (h->traj_mode == 2) {   // general trajectories: segment tables
          if constexpr (CTRL() <= 1)
            k_rollout_traj<T, S, RK4(), DRAG(), CTRL(), COMP, OBS()><<<grid, kBlock, 0, st>>>(
                params<T>(h).c, gain, h->n, h->ld, t0, dt, n_steps, (S*)h->state, (const T*)h->origin, SegTable{h->segs, h->nseg_total}, h->tinfo,
                (T*)rpm_track(h), (S*)obs_log, log_stride, (S*)obs_last, (S*)h->state_lo);
        } else {
          auto* k = &k_rollout_geometric<T, S, RK4(), DRAG(), CTRL(), COMP, OBS()>;
          // the lean loops of a yaw-free handle whose phases repeat from wave to wave read sin / cos of the phase from the handle's table
          if constexpr (CTRL() == 0 && std::is_same_v<S, float> && !RK4() && !DRAG() && COMP == 0 && OBS() >= 0)
            if (use_phase_table(h, n_steps, st)) {
              // ... or, where the amplitudes repeat as well, what the controller reads of the desired state
              const bool wide = use_desired_table(h, n_steps, st);
              const T* rows = (const T*)phase_table_rows(h, t0, dt, n_steps, wide, st);
              auto* const kt = wide ? &k_rollout_geometric_y0d<T, S, false, false, 0, OBS()> : &k_rollout_geometric_y0p<T, S, false, false, 0, OBS()>;
              kt<<<grid, kBlock, 0, st>>>(params<T>(h).c, gain, h->n, h->ld, t0, dt, n_steps, (S*)h->state, (const T*)h->lem, (T*)rpm_track(h),
                                          (S*)obs_log, log_stride, (S*)obs_last, (T*)h->ll, (const S*)obs_last, (S*)h->state_lo, rows);
              h->last_rollout_phase_table = 1;
              h->last_rollout_desired_table = wide ? 1 : 0;
              return;
            }
          if constexpr (CTRL() == 0)
            if (use_yaw_free(h)) k = &k_rollout_geometric_y0<T, S, RK4(), DRAG(), COMP, OBS()>;
          k<<<grid, kBlock, 0, st>>>(params<T>(h).c, gain, h->n, h->ld, t0, dt, n_steps, (S*)h->state, (const T*)h->lem, (T*)rpm_track(h), (S*)obs_log,
                                     log_stride, (S*)obs_last, (T*)h->ll, (const S*)obs_last, (S*)h->state_lo);
        }
      };
      // The kernels take the compensated storage (COMP: MDS_F32C handles) and the destination of the rows (OBS) as template arguments.  The
      // fp32-arithmetic Euler / no-drag GeometricControl loops (the bench's headline among them) are instantiated per destination; the other
      // combinations (RK4, drag, the LQR family, float64) take it at run time (OBS -1), as before: their register budget is set by the
      // arithmetic, not by the three expansions of the row writer, and the library would otherwise carry three copies of each.
      constexpr bool kPerObs = sizeof(T) == 4 && !RK4() && !DRAG() && CTRL() == 0;
      if constexpr (kPerObs) with_int<kObsInPlace, kObsLog, kObsLast>(omode, roll);
      else roll(std::integral_constant<int, -1>{});
    }, h->cfg.integrator == MDS_INTEGRATOR_RK4, has_drag(h));
  };
  // the LQR-omega / LQR-yank-omega loops are built for f32 / f32c / f64 only; GeometricControl and the 12-state LQR also for fp16 storage
  if (ctrl >= 2) with_int<2, 3>(ctrl, [&](auto CTRL) { with_dtype_no_half(h->cfg.dtype, [&](auto DT) { launch(DT, CTRL); }); });
  else with_int<1, 0>(ctrl, [&](auto CTRL) { with_dtype(h->cfg.dtype, [&](auto DT) { launch(DT, CTRL); }); });
}

int mds_rollout_geometric(mds_handle* h, double t0, int n_steps, void* obs, int obs_every_step, void* stream) {
  MDS_DEV(h);
  if (!h || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_geometric");
  if (!h->has_traj) return fail(MDS_ESTATE, "mds_rollout_geometric: call mds_set_lemniscate first");
  if (!aligned16(obs)) return fail(MDS_EALIGN, "mds_rollout_geometric: obs_dev");
  hipStream_t st = (hipStream_t)stream;
  const double dt = 1.0 / h->cfg.ctrl_freq;
  if (rollout_form_policy(h, n_steps) == 2) {
    // launch-bound shard sizes: the same loop through the whole-rollout kernel, rollout_chunk control steps per launch; every step's
    // observation overwrites obs (obs_every_step) exactly as the per-step loop's launches do, or only the last step's is written
    h->last_rollout_streams = 1;
    h->last_rollout_form = 2;
    for (Chunks c{n_steps, h->rollout_chunk, t0, dt, 0, 0}; c.k < n_steps; c.advance(c.len())) {
      const bool last = c.k + c.len() == n_steps;
      launch_rollout_kernel(h, 0, c.t, c.len(), obs_every_step ? obs : nullptr, 0, (!obs_every_step && last) ? obs : nullptr, st);
    }
    return check_launches();
  }
  if (!h->envfx) h->last_rollout_form = 1;       // (ground effect / downwash handles have no launch form: they keep reporting 0)
  // Drones never read each other's rows in this kernel, so the two halves of a big shard are two independent step chains.  Run on
  // two streams they drift out of phase: one half's load/store bursts fill the other's compute phase (measured on C3: 17.5 ->
  // 15.7-16.3 us per step).  The caller's stream orders both chains.
  double t = t0;
  auto step = [&](int k, const Chain* ch, int nc) -> int {
    void* o = (obs_every_step || k == n_steps - 1) ? obs : nullptr;
    for (int c = 0; c < nc; ++c)
      if (int rc = step_geometric(h, t, o, nullptr, ch[c])) return rc;
    t += dt;          // t accumulates exactly like the reference loop (t += env.CTRL_TIMESTEP, EnvGeometric.py:473)
    return MDS_OK;
  };
  return step_loop_batches(h, st, 0, n_steps, step);
}

// what mds_rollout_step and mds_rollout_step_fused ask of their arguments
static int rollout_step_args(const mds_handle* h, const char* who, const void* actions, int n_action_sets, int first_step, int n_steps,
                             const void* obs_log, int log_slots, int episode_len) {
  if (!h || !actions || n_action_sets < 1 || first_step < 0 || n_steps < 0 || (obs_log && log_slots < 1) || episode_len < 0)
    return fail(MDS_EINVAL, who, ": arguments");
  if (episode_len > 0 && !h->init_pose) return fail(MDS_ESTATE, who, ": episode resets need an earlier mds_reset");
  const size_t es = elem_size(h->cfg.dtype), act_bytes = (size_t)h->n * 4 * es, obs_bytes = (size_t)h->n * kObsDim * es;
  if (!aligned16(actions) || !aligned16(obs_log) || (n_action_sets > 1 && act_bytes % 16) || (obs_log && log_slots > 1 && obs_bytes % 16))
    return fail(MDS_EALIGN, who, ": actions_dev/obs_log_dev (every action set and log slot must start 16-byte aligned)");
  return MDS_OK;
}

int mds_rollout_step(mds_handle* h, const void* actions, int n_action_sets, int first_step, int n_steps, void* obs_log, int log_slots,
                     int episode_len, void* stream) {
  MDS_DEV(h);
  if (int rc = rollout_step_args(h, "mds_rollout_step", actions, n_action_sets, first_step, n_steps, obs_log, log_slots, episode_len)) return rc;
  const size_t es = elem_size(h->cfg.dtype), act_bytes = (size_t)h->n * 4 * es, obs_bytes = (size_t)h->n * kObsDim * es;
  // the two halves of a big shard as independent step chains, as in mds_rollout_geometric
  auto step = [&](int k, const Chain* ch, int nc) -> int {
    const long long j = (long long)first_step + k;
    const char* a = (const char*)actions + (size_t)(j % n_action_sets) * act_bytes;
    char* o = obs_log ? (char*)obs_log + (size_t)(j % log_slots) * obs_bytes : nullptr;
    if (episode_len > 0 && j > 0 && j % episode_len == 0)        // a new episode starts at step j: back to the initial poses
      for (int c = 0; c < nc; ++c) {
        const size_t i0 = (size_t)ch[c].i0 * kBlock, i1 = i0 + (size_t)ch[c].n * kBlock;
        if (int rc = launch_reset_range(h, ch[c].st, i0, ch[c].n && i1 < (size_t)h->n ? i1 : (size_t)h->n)) return rc;
      }
    for (int c = 0; c < nc; ++c)
      if (int rc = step_plain(h, a, o, ch[c])) return rc;
    return MDS_OK;
  };
  return step_loop_batches(h, (hipStream_t)stream, 0, n_steps, step);
}

int mds_rollout_step_fused(mds_handle* h, const void* actions, int n_action_sets, int first_step, int n_steps, void* obs_log,
                           int log_slots, int episode_len, int steps_per_launch, void* stream) {
  MDS_DEV(h);
  if (steps_per_launch < 1) return fail(MDS_EINVAL, "mds_rollout_step_fused: arguments");
  if (h && h->envfx)            // env-mates interact every substep: no state-in-registers form; the step-by-step loop serves it
    return mds_rollout_step(h, actions, n_action_sets, first_step, n_steps, obs_log, log_slots, episode_len, stream);
  if (int rc = rollout_step_args(h, "mds_rollout_step_fused", actions, n_action_sets, first_step, n_steps, obs_log, log_slots, episode_len))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = grid_for(h->n, kBlock);
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  int ks = 0;
  for (Chunks c{n_steps, steps_per_launch, 0.0, 0.0, obs_log ? first_step % log_slots : 0, obs_log ? log_slots : 0}; c.k < n_steps; c.advance(ks)) {
    const long long j = (long long)first_step + c.k;
    ks = c.len();
    if (episode_len > 0) {
      if (j > 0 && j % episode_len == 0)
        if (int rc = launch_reset_range(h, st, 0, h->n)) return rc;
      const long long to_boundary = episode_len - j % episode_len;        // a launch never crosses an episode boundary
      if (ks > to_boundary) ks = (int)to_boundary;
    }
    const int a0 = (int)(j % n_action_sets), s0 = c.slot;
    with_flags([&](auto RK4, auto DRAG) {
      with_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
        k_rollout_step<T, S, RK4(), DRAG()><<<grid, kBlock, 0, st>>>(params<T>(h).c, h->n, h->ld, (S*)h->state, (const T*)h->origin, (T*)rpm_track(h),
                                                                     (const S*)actions, a0, n_action_sets, (S*)obs_log, s0, obs_log ? log_slots : 1,
                                                                     ks, (S*)h->state_lo);
      });
    }, rk4, drag);
  }
  return check_launches();
}

// ---- per-env episodes (mds_episode.hpp, mds_episode_kernels.hip) ----
int mds_default_episode_params(mds_episode_params* p) {
  if (!p) return fail(MDS_EINVAL, "mds_default_episode_params: null argument");
  memset(p, 0, sizeof(*p));
  p->z_min = -(double)INFINITY;
  p->z_max = p->max_dist = p->max_tilt = p->max_speed = p->max_rate = (double)INFINITY;
  p->reward_r0 = 2.0;
  return MDS_OK;
}

int mds_set_episodes(mds_handle* h, const mds_episode_params* p, const double* target_host, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_set_episodes: null handle");
  if (!p) {
    h->ep_on = h->ep_safe = h->ep_random = h->ep_policy = h->ep_noise = false;
    return MDS_OK;
  }
  if (p->max_steps < 0 || !(p->reward_r0 == p->reward_r0) || !(p->term_penalty == p->term_penalty))
    return fail(MDS_EINVAL, "mds_set_episodes: max_steps < 0, or reward_r0 / term_penalty is NaN");
  if (h->cfg.dtype == MDS_F32C || h->envfx || h->cfg.num_drones > kBlock / 2)
    return fail(MDS_EUNSUPPORTED, "mds_set_episodes: built for MDS_F32 / MDS_F64 / MDS_F16 storage, DYN / DYN_DRAG physics and at most 128 drones per env");
  if (!h->init_pose) return fail(MDS_ESTATE, "mds_set_episodes: needs an earlier mds_reset");
  hipStream_t st = (hipStream_t)stream;
  const size_t es = elem_size(h->cfg.dtype), cs = comp_size(h->cfg.dtype), tb = (size_t)h->n * 3 * sizeof(double);
  h->ep_slots = ((size_t)h->cfg.num_envs + 31) / 32 * 32;
  if (int rc = h->mem.alloc_all({{&h->ep_image, 13 * h->ld * es}, {&h->ep_target, 4 * h->ld * cs}, {&h->ep_counters, 5 * h->ep_slots * 8}})) return rc;
  if (target_host) {
    if (int rc = h->mem.alloc(&h->ep_target_world, tb)) return rc;
    MDS_HIP(hipMemcpyAsync(h->ep_target_world, target_host, tb, hipMemcpyHostToDevice, st));
  } else if (h->ep_target_world) {
    MDS_HIP(hipStreamSynchronize(st));          // (set-up path: nothing enqueued may still read it)
    h->mem.release(&h->ep_target_world);
  }
  h->ep = *p;
  if (int rc = episode_build_image(h, st)) return rc;
  MDS_HIP(hipMemsetAsync(h->ep_counters, 0, 5 * h->ep_slots * 8, st));
  if (h->ep_hmin)                      // the running episodes start anew: so do their minima (the safety settings themselves stay)
    if (int rc = episode_hmin_clear(h, st, h->ep_hmin, 1, 1)) return rc;
  h->ep_on = true;
  ++h->ep_epoch;                       // every env's running episode starts anew
  if (target_host) MDS_HIP(hipStreamSynchronize(st));   // host buffer may be reused by the caller
  return MDS_OK;
}

int mds_episode_ptrs(mds_handle* h, void* ptrs[5]) {
  if (!h || !ptrs) return fail(MDS_EINVAL, "mds_episode_ptrs: null argument");
  if (!h->ep_counters) return fail(MDS_ESTATE, "mds_episode_ptrs: no mds_set_episodes yet");
  for (int k = 0; k < 5; ++k) ptrs[k] = (char*)h->ep_counters + (size_t)k * h->ep_slots * 8;
  return MDS_OK;
}

static_assert(MDS_EPISODE_MAX_OBSTACLES == kEpMaxObstacles, "include/mds.h and mds_episode.hpp disagree");

int mds_set_episode_safety(mds_handle* h, const mds_episode_safety* p, const double* obstacles_host, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_set_episode_safety: null handle");
  if (!p) {
    h->ep_safe = false;
    return MDS_OK;
  }
  auto positive = [](double x) { return x > 0.0 && x < (double)INFINITY; };
  if (!positive(p->safety_radius) || !positive(p->zscale) || p->n_obs < 0 || p->n_obs > MDS_EPISODE_MAX_OBSTACLES || (p->n_obs > 0 && !obstacles_host))
    return fail(MDS_EINVAL, "mds_set_episode_safety: safety_radius and zscale must be finite and > 0, n_obs in 0..16 with its obstacle list");
  for (int k = 0; k < 4 * p->n_obs; ++k) {
    const double v = obstacles_host[k];
    if (!(v > -(double)INFINITY && v < (double)INFINITY) || (k % 4 == 3 && v < 0.0))
      return fail(MDS_EINVAL, "mds_set_episode_safety: an obstacle value is not finite, or a radius is negative");
  }
  if (!h->ep_on) return fail(MDS_ESTATE, "mds_set_episode_safety: no episodes configured (mds_set_episodes)");
  hipStream_t st = (hipStream_t)stream;
  // a first call allocates the two arrays; every call puts both back to +inf (a minimum over another set says nothing about this one).
  // The handle's settings change only once that has been enqueued: a failure before leaves them, and a fresh block is given back.
  const bool fresh = !h->ep_hmin;
  if (int rc = h->mem.alloc(&h->ep_hmin, 2 * h->ep_slots * 8)) return rc;
  if (int rc = episode_hmin_clear(h, st, h->ep_hmin, 0, 2)) {
    if (fresh) h->mem.release(&h->ep_hmin);
    return rc;
  }
  h->ep_safety = *p;
  h->ep_safety.reserved = 0;
  memset(h->ep_obstacles, 0, sizeof(h->ep_obstacles));
  if (p->n_obs > 0) memcpy(h->ep_obstacles, obstacles_host, (size_t)p->n_obs * 4 * sizeof(double));
  h->ep_safe = true;
  return MDS_OK;
}

int mds_episode_safety_ptrs(mds_handle* h, void* ptrs[2]) {
  if (!h || !ptrs) return fail(MDS_EINVAL, "mds_episode_safety_ptrs: null argument");
  if (!h->ep_hmin) return fail(MDS_ESTATE, "mds_episode_safety_ptrs: no mds_set_episode_safety yet");
  for (int k = 0; k < 2; ++k) ptrs[k] = (char*)h->ep_hmin + (size_t)k * h->ep_slots * 8;
  return MDS_OK;
}

int mds_set_episode_randomisation(mds_handle* h, const mds_episode_randomisation* p, void* stream) {
  (void)stream;                        // (nothing is enqueued: the parameters travel with the launches)
  if (!h) return fail(MDS_EINVAL, "mds_set_episode_randomisation: null handle");
  if (!p) {
    h->ep_random = false;
    return MDS_OK;
  }
  const double* groups[4] = {p->pos, p->rpy, p->vel, p->rate};
  for (const double* g : groups)
    for (int k = 0; k < 3; ++k)
      if (!(g[k] >= 0.0 && g[k] < (double)INFINITY))
        return fail(MDS_EINVAL, "mds_set_episode_randomisation: a half-width is not finite or is negative");
  // g = first_env * D + i is a 32-bit counter word: the whole shard must fit
  const unsigned long long E = (unsigned long long)h->cfg.num_envs, D = (unsigned long long)h->cfg.num_drones;
  if (p->first_env < 0 || (unsigned long long)p->first_env > 0xFFFFFFFFull || ((unsigned long long)p->first_env + E) * D > 0xFFFFFFFFull)
    return fail(MDS_EINVAL, "mds_set_episode_randomisation: first_env < 0, or (first_env + num_envs) * num_drones does not fit 32 bits");
  if (!h->ep_on) return fail(MDS_ESTATE, "mds_set_episode_randomisation: no episodes configured (mds_set_episodes)");
  h->ep_rand = *p;
  h->ep_generation = 0;
  h->ep_random = true;
  return MDS_OK;
}

int mds_reset_episodes(mds_handle* h, void* obs, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_reset_episodes: null handle");
  if (!aligned16(obs)) return fail(MDS_EALIGN, "mds_reset_episodes: obs_dev");
  if (!h->ep_on || !h->ep_random) return fail(MDS_ESTATE, "mds_reset_episodes: no randomisation configured (mds_set_episode_randomisation)");
  hipStream_t st = (hipStream_t)stream;
  ++h->ep_generation;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_episode_reset_random<T, S><<<grid_for(h->n, kBlock), kBlock, 0, st>>>(
        h->n, h->ld, h->cfg.num_drones, episode_random_args<T>(h), (const int*)((char*)h->ep_counters + 2 * h->ep_slots * 8),
        (const S*)h->ep_image, (const T*)h->origin, (S*)h->state, (T*)h->last_rpm, (S*)obs);
  });
  MDS_HIP(hipGetLastError());
  h->rpm_stale = false;
  return episode_restart(h, st);
}

int mds_rollout_episodes(mds_handle* h, const void* actions, int n_action_sets, int first_step, int n_steps, void* obs_log, int log_slots,
                         void* reward_log, int32_t* flags_log, int steps_per_launch, void* obs, void* stream) {
  MDS_DEV(h);
  const bool ring = obs_log || reward_log || flags_log;
  if (steps_per_launch < 1 || (ring && log_slots < 1)) return fail(MDS_EINVAL, "mds_rollout_episodes: arguments");
  if (int rc = rollout_step_args(h, "mds_rollout_episodes", actions, n_action_sets, first_step, n_steps, obs_log, log_slots, 0)) return rc;
  if (!aligned16(obs) || !aligned16(reward_log) || !aligned16(flags_log))
    return fail(MDS_EALIGN, "mds_rollout_episodes: obs_dev/reward_log_dev/flags_log_dev");
  if (!h->ep_on) return fail(MDS_ESTATE, "mds_rollout_episodes: no episodes configured (mds_set_episodes)");
  hipStream_t st = (hipStream_t)stream;
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  for (Chunks c{n_steps, steps_per_launch, 0.0, 0.0, ring ? first_step % log_slots : 0, ring ? log_slots : 0}; c.k < n_steps; c.advance(c.len())) {
    const int ks = c.len(), a0 = (int)(((long long)first_step + c.k) % n_action_sets), s0 = c.slot;
    const bool last = c.k + ks == n_steps;
    with_flags([&](auto RK4, auto DRAG) {
      with_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
        const EpisodeLaunch<T> ep = episode_launch<T>(h);
        // one launch, whichever of the four kernels: `extra` is what follows the counters (nothing | the safety set | the
        // randomisation | both, in this order)
        auto launch = [&](auto kernel, auto... extra) {
          kernel<<<ep.grid, kBlock, 0, st>>>(params<T>(h).c, ep.rule, h->n, h->ld, ep.D, ep.epb, (S*)h->state, (const S*)h->ep_image,
                                             (const T*)h->origin, (const T*)h->ep_target, (T*)rpm_track(h), (const S*)actions, a0, n_action_sets,
                                             (S*)obs_log, (T*)reward_log, (int*)flags_log, s0, ring ? log_slots : 1, ks, (S*)(last ? obs : nullptr),
                                             ep.cnt, extra...);
        };
        using R = EpisodeRandomArgs<T>;
        if (h->ep_safe && h->ep_random) launch(k_rollout_episodes_safe<T, S, RK4(), DRAG(), R>, ep.safe, ep.rnd);
        else if (h->ep_safe) launch(k_rollout_episodes_safe<T, S, RK4(), DRAG()>, ep.safe);
        else if (h->ep_random) launch(k_rollout_episodes<T, S, RK4(), DRAG(), R>, ep.rnd);
        else launch(k_rollout_episodes<T, S, RK4(), DRAG()>);
      });
    }, rk4, drag);
  }
  return check_launches();
}

int mds_step_episodes(mds_handle* h, const void* action, void* obs, void* final_obs, void* reward, int32_t* flags, void* stream) {
  if (!h || !action) return fail(MDS_EINVAL, "mds_step_episodes: null argument");
  return mds_rollout_episodes(h, action, 1, 0, 1, final_obs, 1, reward, flags, 1, obs, stream);
}

// ---- an MLP policy inside the episode rollout kernel (mds_policy.hpp, mds_episode_policy_kernels.hip) ----
static_assert(sizeof(mds_episode_policy) == 32, "include/mds.h mds_episode_policy: four int32 and two doubles");

int mds_set_episode_policy(mds_handle* h, const mds_episode_policy* p, const double* weights_host, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_set_episode_policy: null handle");
  if (!p) {
    h->ep_policy = h->ep_noise = false;
    return MDS_OK;
  }
  auto finite = [](double x) { return x > -(double)INFINITY && x < (double)INFINITY; };
  auto finite_or_nan = [&](double x) { return !(x == x) || finite(x); };
  if (p->n_hidden < 1 || p->n_hidden > 2 || p->width < 1 || p->width > kPolicyMaxWidth || p->activation < 0 || p->activation > 1 || !weights_host ||
      !finite_or_nan(p->rpm_base) || !finite_or_nan(p->rpm_scale))
    return fail(MDS_EINVAL, "mds_set_episode_policy: n_hidden in 1..2, width in 1..64, activation 0 or 1, weights, rpm_base / rpm_scale finite or NaN");
  const int nw = policy_n_weights(p->n_hidden, p->width);
  for (int k = 0; k < nw; ++k)
    if (!finite(weights_host[k])) return fail(MDS_EINVAL, "mds_set_episode_policy: a weight is not finite");
  if (h->cfg.dtype == MDS_F32C || h->cfg.dtype == MDS_F16 || h->envfx || h->cfg.num_drones > kBlock / 2)
    return fail(MDS_EUNSUPPORTED, "mds_set_episode_policy: built for MDS_F32 / MDS_F64, DYN / DYN_DRAG physics and at most 128 drones per env");
  if (!h->ep_on) return fail(MDS_ESTATE, "mds_set_episode_policy: no episodes configured (mds_set_episodes)");
  hipStream_t st = (hipStream_t)stream;
  // the padded weights in the compute type, built on the host; the new block is filled before the old one is given up (DevMem::replace),
  // and the handle's settings change only after that
  // (float64 with the RK4 integrator has no 32-wide rollout kernel, see mds_rollout_episodes_policy: the 64-wide one serves, same bits)
  const bool wide_only = h->cfg.dtype == MDS_F64 && h->cfg.integrator == MDS_INTEGRATOR_RK4;
  const int W = wide_only ? kPolicyWidths[1] : policy_device_width(p->width), nw_pad = policy_n_weights(p->n_hidden, W);
  const size_t cs = comp_size(h->cfg.dtype);
  std::vector<double> padded((size_t)nw_pad), w64((size_t)nw_pad);
  std::vector<float> w32(cs == 4 ? (size_t)nw_pad : 0);
  policy_pad(weights_host, p->n_hidden, p->width, W, padded.data());
  policy_device_layout(padded.data(), p->n_hidden, W, w64.data());
  for (size_t k = 0; k < w32.size(); ++k) w32[k] = (float)w64[k];
  for (size_t k = 0; k < w32.size(); ++k)
    if (!finite((double)w32[k])) return fail(MDS_EINVAL, "mds_set_episode_policy: a weight is not finite in float32");
  const void* src = cs == 4 ? (const void*)w32.data() : (const void*)w64.data();
  MDS_HIP(hipStreamSynchronize(st));          // (set-up path: nothing enqueued may still read the old block)
  if (int rc = h->mem.replace(&h->ep_policy_w, (size_t)nw_pad * cs, [&](void* fresh) {
        return dev_status(hipMemcpy(fresh, src, (size_t)nw_pad * cs, hipMemcpyHostToDevice), "mds_set_episode_policy: upload");
      }))
    return rc;
  h->ep_pol = *p;
  h->ep_pol.reserved = 0;
  const double hover = sqrt(h->cfg.G * h->cfg.M / (4.0 * h->cfg.KF));
  if (!(p->rpm_base == p->rpm_base)) h->ep_pol.rpm_base = hover;
  if (!(p->rpm_scale == p->rpm_scale)) h->ep_pol.rpm_scale = 0.05 * hover;
  h->ep_policy_width = W;
  h->ep_policy = true;
  return MDS_OK;
}

int mds_episode_policy_compute(mds_handle* h, const void* obs, void* rpm, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !rpm) return fail(MDS_EINVAL, "mds_episode_policy_compute: null argument");
  if (!aligned16(obs) || !aligned16(rpm)) return fail(MDS_EALIGN, "mds_episode_policy_compute: obs_dev/rpm_dev");
  if (!h->ep_on || !h->ep_policy) return fail(MDS_ESTATE, "mds_episode_policy_compute: no policy configured (mds_set_episode_policy)");
  hipStream_t st = (hipStream_t)stream;
  with_policy_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    with_int<32, 64>(h->ep_policy_width, [&](auto W) {
      k_episode_policy_compute<T, S, W()><<<grid_for(h->n, kBlock), kBlock, 0, st>>>(h->n, h->ld, (const T*)h->origin, (const T*)h->ep_target,
                                                                                     episode_policy_args<T>(h), (const S*)obs, (S*)rpm);
    });
  });
  return check_launches();
}

int mds_rollout_episodes_policy(mds_handle* h, int first_step, int n_steps, void* obs_log, int log_slots, void* action_log, void* reward_log,
                                int32_t* flags_log, int steps_per_launch, void* obs, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_rollout_episodes_policy: null handle");
  const bool ring = obs_log || action_log || reward_log || flags_log;
  if (steps_per_launch < 1 || first_step < 0 || n_steps < 0 || (ring && log_slots < 1)) return fail(MDS_EINVAL, "mds_rollout_episodes_policy: arguments");
  if (!aligned16(obs) || !aligned16(obs_log) || !aligned16(action_log) || !aligned16(reward_log) || !aligned16(flags_log))
    return fail(MDS_EALIGN, "mds_rollout_episodes_policy: obs_dev/obs_log_dev/action_log_dev/reward_log_dev/flags_log_dev");
  if (!h->ep_on || !h->ep_policy) return fail(MDS_ESTATE, "mds_rollout_episodes_policy: no policy configured (mds_set_episodes, mds_set_episode_policy)");
  hipStream_t st = (hipStream_t)stream;
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  for (Chunks c{n_steps, steps_per_launch, 0.0, 0.0, ring ? first_step % log_slots : 0, ring ? log_slots : 0}; c.k < n_steps; c.advance(c.len())) {
    const int ks = c.len(), s0 = c.slot;
    const bool last = c.k + ks == n_steps;
    with_flags([&](auto RK4, auto DRAG) {
      with_policy_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
        const EpisodeLaunch<T> ep = episode_launch<T>(h);
        with_int<32, 64>(h->ep_policy_width, [&](auto W) {
          // not built: float64, RK4, 32 wide -- the one combination whose register allocation leaves a (never accessed) slot in the private
          // segment; mds_set_episode_policy pads such a handle's policy to 64, which changes no bit
          if constexpr (!(RK4() && sizeof(T) == 8 && W() == 32))
          k_rollout_episodes_policy<T, S, RK4(), DRAG(), W()><<<ep.grid, kBlock, 0, st>>>(
              params<T>(h).c, ep.rule, h->n, h->ld, ep.D, ep.epb, (S*)h->state, (const S*)h->ep_image, (const T*)h->origin, (const T*)h->ep_target,
              (T*)rpm_track(h), episode_policy_args<T>(h), (S*)action_log, (S*)obs_log, (T*)reward_log, (int*)flags_log, s0, ring ? log_slots : 1, ks,
              (S*)(last ? obs : nullptr), ep.cnt, h->ep_safe ? 1 : 0, ep.safe, h->ep_random ? 1 : 0, ep.rnd);
        });
      });
    }, rk4, drag);
  }
  return check_launches();
}

// ---- Gaussian actions drawn in the rollout kernel (mds_policy_noise.hpp, mds_episode_sample_kernels.hip) ----
static_assert(sizeof(mds_episode_policy_noise) == 48, "include/mds.h mds_episode_policy_noise: a uint64, an int64 and four doubles");
static_assert(sizeof(mds_episode_sample_rings) == 7 * sizeof(void*), "include/mds.h mds_episode_sample_rings: seven pointers");

int mds_set_episode_policy_noise(mds_handle* h, const mds_episode_policy_noise* p, void* stream) {
  (void)stream;                        // (nothing is enqueued: the parameters travel with the launches)
  if (!h) return fail(MDS_EINVAL, "mds_set_episode_policy_noise: null handle");
  if (!p) {
    h->ep_noise = false;
    return MDS_OK;
  }
  // sigma must be a normal number of the compute type (compared in double, nothing out of range is converted; a denormal counts as 0:
  // the device may flush it)
  const bool f64 = h->cfg.dtype == MDS_F64;
  const double lo = f64 ? DBL_MIN : (double)FLT_MIN, hi = f64 ? DBL_MAX : (double)FLT_MAX;
  for (int j = 0; j < 4; ++j) {
    const double ls = p->log_std[j], sd = exp(ls);
    if (!(ls > -(double)INFINITY && ls < (double)INFINITY) || !(sd >= lo && sd <= hi))
      return fail(MDS_EINVAL, "mds_set_episode_policy_noise: a log_std is not finite, or its exp is 0 or infinite in the compute type");
  }
  // g = first_env * D + i is a 32-bit counter word: the whole shard must fit
  const unsigned long long E = (unsigned long long)h->cfg.num_envs, D = (unsigned long long)h->cfg.num_drones;
  if (p->first_env < 0 || (unsigned long long)p->first_env > 0xFFFFFFFFull || ((unsigned long long)p->first_env + E) * D > 0xFFFFFFFFull)
    return fail(MDS_EINVAL, "mds_set_episode_policy_noise: first_env < 0, or (first_env + num_envs) * num_drones does not fit 32 bits");
  if (!h->ep_on || !h->ep_policy) return fail(MDS_ESTATE, "mds_set_episode_policy_noise: no policy configured (mds_set_episodes, mds_set_episode_policy)");
  h->ep_noise_p = *p;
  h->ep_epoch = 0;
  h->ep_noise = true;
  return MDS_OK;
}

int mds_episode_policy_sample(mds_handle* h, const void* obs, void* rpm, void* sample, void* logp, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !rpm) return fail(MDS_EINVAL, "mds_episode_policy_sample: null argument");
  if (!aligned16(obs) || !aligned16(rpm) || !aligned16(sample) || !aligned16(logp))
    return fail(MDS_EALIGN, "mds_episode_policy_sample: obs_dev/rpm_dev/sample_dev/logp_dev");
  if (!h->ep_on || !h->ep_policy || !h->ep_noise)
    return fail(MDS_ESTATE, "mds_episode_policy_sample: no policy noise configured (mds_set_episode_policy, mds_set_episode_policy_noise)");
  hipStream_t st = (hipStream_t)stream;
  const char* cb = (const char*)h->ep_counters;
  const size_t sl = h->ep_slots * 8;
  with_policy_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    with_int<32, 64>(h->ep_policy_width, [&](auto W) {
      k_episode_policy_sample<T, S, W()><<<grid_for(h->n, kBlock), kBlock, 0, st>>>(
          h->n, h->ld, h->cfg.num_drones, (const T*)h->origin, (const T*)h->ep_target, episode_policy_args<T>(h), episode_noise_args<T>(h),
          (const int*)(cb + 2 * sl), (const int*)cb, (const S*)obs, (S*)rpm, (S*)sample, (T*)logp);
    });
  });
  return check_launches();
}

int mds_rollout_episodes_sampled(mds_handle* h, int first_step, int n_steps, const mds_episode_sample_rings* rings, int log_slots,
                                 int steps_per_launch, void* obs, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_rollout_episodes_sampled: null handle");
  const mds_episode_sample_rings none = {};
  const mds_episode_sample_rings& R = rings ? *rings : none;
  const bool ring = R.acted_obs || R.obs || R.action || R.sample || R.logp || R.reward || R.flags;
  if (steps_per_launch < 1 || first_step < 0 || n_steps < 0 || (ring && log_slots < 1)) return fail(MDS_EINVAL, "mds_rollout_episodes_sampled: arguments");
  if (!aligned16(obs) || !aligned16(R.acted_obs) || !aligned16(R.obs) || !aligned16(R.action) || !aligned16(R.sample) || !aligned16(R.logp) ||
      !aligned16(R.reward) || !aligned16(R.flags))
    return fail(MDS_EALIGN, "mds_rollout_episodes_sampled: obs_dev or a ring");
  if (!h->ep_on || !h->ep_policy || !h->ep_noise)
    return fail(MDS_ESTATE, "mds_rollout_episodes_sampled: no policy noise configured (mds_set_episode_policy, mds_set_episode_policy_noise)");
  hipStream_t st = (hipStream_t)stream;
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  for (Chunks c{n_steps, steps_per_launch, 0.0, 0.0, ring ? first_step % log_slots : 0, ring ? log_slots : 0}; c.k < n_steps; c.advance(c.len())) {
    const int ks = c.len(), s0 = c.slot;
    const bool last = c.k + ks == n_steps;
    // the RPM planes carry the echo from launch to launch (the acted-on rows of a launch's first step read it): NaN where they are
    // not current (what mds_get_obs reports then), always written -- which makes them current
    if (!h->track_rpm && h->rpm_stale) {
      const size_t count = 4 * h->ld;
      with_policy_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T;
        k_episode_echo_unknown<T><<<dim3((unsigned)((count + kBlock - 1) / kBlock)), kBlock, 0, st>>>(count, (T*)h->last_rpm);
      });
    }
    with_flags([&](auto RK4, auto DRAG) {
      with_policy_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
        const EpisodeLaunch<T> ep = episode_launch<T>(h);
        const EpisodeSampleRings<T, S> rg = {(S*)R.acted_obs, (S*)R.obs, (S*)R.action, (S*)R.sample, (T*)R.logp, (T*)R.reward, (int*)R.flags};
        with_int<32, 64>(h->ep_policy_width, [&](auto W) {
          // (float64, RK4, 32 wide is not built, as in mds_rollout_episodes_policy: mds_set_episode_policy pads such a handle's policy to 64)
          if constexpr (!(RK4() && sizeof(T) == 8 && W() == 32))
          k_rollout_episodes_sampled<T, S, RK4(), DRAG(), W()><<<ep.grid, kBlock, 0, st>>>(
              params<T>(h).c, ep.rule, h->n, h->ld, ep.D, ep.epb, (S*)h->state, (const S*)h->ep_image, (const T*)h->origin, (const T*)h->ep_target,
              (T*)h->last_rpm, episode_policy_args<T>(h), episode_noise_args<T>(h), rg, s0, ring ? log_slots : 1, ks,
              (S*)(last ? obs : nullptr), ep.cnt, h->ep_safe ? 1 : 0, ep.safe, h->ep_random ? 1 : 0, ep.rnd);
        });
      });
    }, rk4, drag);
    h->rpm_stale = false;
  }
  return check_launches();
}

int mds_set_rollout_streams(mds_handle* h, int n_streams) {
  if (!h || n_streams < 0 || n_streams > 2) return fail(MDS_EINVAL, "mds_set_rollout_streams: 0 (auto), 1 or 2");
  MDS_DEV(h);
  if (n_streams == 2)          // a set-up call: the only place besides mds_create that creates the internal streams
    if (int rc = split_streams_ready(h)) return rc;
  h->rollout_streams = n_streams;
  return MDS_OK;
}

int mds_rollout_streams_for(const mds_handle* h, int loop, int n_steps) {
  if (!h || loop < 0 || loop > 1 || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_streams_for");
  return rollout_streams_policy(h, loop, n_steps);
}

int mds_get_last_rollout_streams(const mds_handle* h) {
  if (!h) return fail(MDS_EINVAL, "mds_get_last_rollout_streams: null handle");
  return h->last_rollout_streams;
}

int mds_set_rollout_form(mds_handle* h, int form, int steps_per_launch) {
  if (!h || form < 0 || form > 2 || steps_per_launch < 0) return fail(MDS_EINVAL, "mds_set_rollout_form: form 0 (auto), 1 or 2; steps_per_launch >= 0 (0: keep)");
  h->rollout_form = form;
  if (steps_per_launch > 0) h->rollout_chunk = steps_per_launch;
  return MDS_OK;
}

int mds_rollout_form_for(const mds_handle* h, int n_steps) {
  if (!h || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_form_for");
  return rollout_form_policy(h, n_steps);
}

int mds_get_last_rollout_form(const mds_handle* h) {
  if (!h) return fail(MDS_EINVAL, "mds_get_last_rollout_form: null handle");
  return h->last_rollout_form;
}

// ctrl: 0 GeometricControl, 1 LQRController (12-state), 2 LQROmegaController + ThrustOmega, 3 LQRYankOmegaController + YankOmega
int rollout_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs_last, void* stream, int ctrl, const char* who) {
  if (!h || n_steps < 0) return fail(MDS_EINVAL, who);
  if (!h->has_traj) return fail(MDS_ESTATE, "mds_rollout_*_fused: call mds_set_lemniscate first");
  if (ctrl == 1 && !h->has_lqr12) return fail(MDS_ESTATE, "mds_rollout_lqr_fused: call mds_set_lqr_gain first");
  if (ctrl >= 2) {
    // (ground effect / downwash handles go step by step, below: what their step function does not serve it refuses itself)
    if (h->traj_mode != 1 && !h->envfx) return fail(MDS_EUNSUPPORTED, "mds_rollout_nominal_fused: Lemniscate trajectories only (use mds_step_nominal)");
    if (h->cfg.dtype == MDS_F16) return fail(MDS_EUNSUPPORTED, "mds_rollout_nominal_fused: fp16 storage");
    if (!obs_last) return fail(MDS_EINVAL, "mds_rollout_nominal_fused: obs_dev is required (in: current observation, out: last one)");
  }
  if (!aligned16(obs_log) || !aligned16(obs_last)) return fail(MDS_EALIGN, "mds_rollout_*_fused: obs buffers");
  // step k's rows start n * 20 elements behind step k - 1's and go out in 16-byte chunks: fp16 storage with an odd n is the one case
  // in which a slot of the log can start off a 16-byte boundary
  const size_t obs_bytes = (size_t)h->n * kObsDim * elem_size(h->cfg.dtype);
  if (obs_log && n_steps > 1 && obs_bytes % 16)
    return fail(MDS_EALIGN, "mds_rollout_*_fused: obs_log_dev (every action set and log slot must start 16-byte aligned)");
  hipStream_t st = (hipStream_t)stream;
  if (h->envfx) {
    // ground effect / downwash: env-mates interact every physics substep, so there is no state-in-registers form; the same loop
    // runs step by step (one launch per substep), each step's observation written straight into its slot of the log
    const double dt = 1.0 / h->cfg.ctrl_freq;
    const int streams_before = h->last_rollout_streams;          // (not one of the calls mds_get_last_rollout_streams reports)
    auto step = [&](int k, const Chain* ch, int) -> int {
      char* slot = obs_log ? (char*)obs_log + (size_t)k * obs_bytes : nullptr;
      const bool last = k == n_steps - 1;
      if (ctrl <= 1) {
        void* o = slot ? (void*)slot : (last ? obs_last : nullptr);
        if (int rc = ctrl == 0 ? step_geometric(h, t0, o, nullptr, ch[0]) : step_lqr(h, t0, o, nullptr, st)) return rc;
        if (slot && last && obs_last) MDS_HIP(hipMemcpyAsync(obs_last, slot, obs_bytes, hipMemcpyDeviceToDevice, st));
      } else {
        if (int rc = step_nominal_lowlevel(h, t0, obs_last, nullptr, nullptr, st)) return rc;
        if (slot) MDS_HIP(hipMemcpyAsync(slot, obs_last, obs_bytes, hipMemcpyDeviceToDevice, st));
      }
      t0 += dt;
      return MDS_OK;
    };
    const int rc = step_loop(h, st, 1, 0, 0, 0, n_steps, step);
    h->last_rollout_streams = streams_before;
    return rc;
  }
  if (n_steps == 0) return MDS_OK;
  launch_rollout_kernel(h, ctrl, t0, n_steps, obs_log, (size_t)h->n * kObsDim, obs_last, st);
  return check_launches();
}

int mds_rollout_geometric_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs_last, void* stream) {
  MDS_DEV(h);
  return rollout_fused(h, t0, n_steps, obs_log, obs_last, stream, 0, "mds_rollout_geometric_fused");
}

int mds_rollout_lqr_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs_last, void* stream) {
  MDS_DEV(h);
  return rollout_fused(h, t0, n_steps, obs_log, obs_last, stream, 1, "mds_rollout_lqr_fused");
}

int mds_rollout_nominal_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_rollout_nominal_fused: null handle");
  if (h->cbf_nominal != 1 && h->cbf_nominal != 2)
    return fail(MDS_ESTATE, "mds_rollout_nominal_fused: select the LQR-omega (1) or LQR-yank-omega (2) controller with mds_cbf_set_nominal first");
  return rollout_fused(h, t0, n_steps, obs_log, obs, stream, h->cbf_nominal == 1 ? 2 : 3, "mds_rollout_nominal_fused");
}

int mds_lemniscate_eval(mds_handle* h, double t, void* des, void* stream) {
  MDS_DEV(h);
  if (!h || !des) return fail(MDS_EINVAL, "mds_lemniscate_eval: null argument");
  if (!h->has_traj || h->traj_mode != 1) return fail(MDS_ESTATE, "mds_lemniscate_eval: call mds_set_lemniscate first");
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_lemniscate_eval<T, S><<<grid_for(h->n, 256), 256, 0, (hipStream_t)stream>>>(h->n, h->ld, t, (const T*)h->lem, (S*)des);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_geometric_compute(mds_handle* h, const void* obs, const void* des, void* rpm, void* aux, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !des || !rpm) return fail(MDS_EINVAL, "mds_geometric_compute: null argument");
  if (!aligned16(rpm)) return fail(MDS_EALIGN, "mds_geometric_compute: rpm_dev");
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_geometric_compute<T, S><<<grid_for(h->n, 256), 256, 0, (hipStream_t)stream>>>(params<T>(h).c, h->n, (const S*)obs, (const S*)des, (S*)rpm, (S*)aux);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_input_to_action(mds_handle* h, const void* u, void* rpm, void* stream) {
  MDS_DEV(h);
  if (!h || !u || !rpm) return fail(MDS_EINVAL, "mds_input_to_action: null argument");
  if (!aligned16(u) || !aligned16(rpm)) return fail(MDS_EALIGN, "mds_input_to_action");
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_input_to_action<T, S><<<grid_for(h->n, 256), 256, 0, (hipStream_t)stream>>>(params<T>(h).c, h->n, (const S*)u, (S*)rpm);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_obs_to_model(mds_handle* h, const void* obs, int dim, void* x, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !x) return fail(MDS_EINVAL, "mds_obs_to_model: null argument");
  if (dim != 9 && dim != 10 && dim != 12 && dim != 18) return fail(MDS_EINVAL, "mds_obs_to_model: dim must be 9, 10, 12 (linear models) or 18 (geometric model)");
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_obs_to_model<T, S><<<grid_for(h->n, 256), 256, 0, (hipStream_t)stream>>>(params<T>(h).c, h->n, dim, (const S*)obs, (S*)x);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_action_to_input(mds_handle* h, const void* rpm, int cap_rpm, void* u, void* stream) {
  MDS_DEV(h);
  if (!h || !u || !rpm) return fail(MDS_EINVAL, "mds_action_to_input: null argument");
  if (!aligned16(u) || !aligned16(rpm)) return fail(MDS_EALIGN, "mds_action_to_input");
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_action_to_input<T, S><<<grid_for(h->n, 256), 256, 0, (hipStream_t)stream>>>(params<T>(h).c, h->n, cap_rpm, (const S*)rpm, (S*)u);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_quadrotor_dynamics(int dtype, int count, const void* state, const void* u, double m, const double J[3], double g,
                           void* out, void* stream) {
  if (count < 0 || !state || !u || !out || !J) return fail(MDS_EINVAL, "mds_quadrotor_dynamics: bad argument");
  if (count == 0) return MDS_OK;
  if (dtype != MDS_F32 && dtype != MDS_F64 && dtype != MDS_F16) return fail(MDS_EINVAL, "mds_quadrotor_dynamics: dtype");
  with_dtype(dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_quadrotor_dynamics<T, S><<<grid_for(count, 256), 256, 0, (hipStream_t)stream>>>(count, (const S*)state, (const S*)u, (T)m, (T)J[0], (T)J[1],
                                                                                       (T)J[2], (T)g, (S*)out);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_compare_models(mds_handle* h, int count, const void* obs, const double* A, const double* B, double u_eq0, double dyn_m,
                       const double dyn_J[3], double dyn_g, void* xdot_lin, void* xdot_geo, void* x_lin, void* stream) {
  MDS_DEV(h);
  if (!h || count < 0 || !obs || !A || !B || !dyn_J) return fail(MDS_EINVAL, "mds_compare_models: bad argument");
  if (!xdot_lin && !xdot_geo && !x_lin) return fail(MDS_EINVAL, "mds_compare_models: no output requested");
  if (!aligned16(obs) || !aligned16(xdot_lin) || !aligned16(xdot_geo) || !aligned16(x_lin)) return fail(MDS_EALIGN, "mds_compare_models");
  if (count == 0) return MDS_OK;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    launch_compare_models<T, S>(params<T>(h).c, count, obs, A, B, u_eq0, dyn_m, dyn_J, dyn_g, xdot_lin, xdot_geo, x_lin, (hipStream_t)stream);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_linear_xdot(mds_handle* h, int count, const void* x, const void* action, const double* A, const double* B, double u_eq0, void* xdot,
                    void* stream) {
  MDS_DEV(h);
  if (!h || count < 0 || !x || !action || !A || !B || !xdot) return fail(MDS_EINVAL, "mds_linear_xdot: bad argument");
  if (count == 0) return MDS_OK;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    launch_linear_xdot<T, S>(params<T>(h).c, count, x, action, A, B, u_eq0, xdot, (hipStream_t)stream);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_rpy_to_rot(int dtype, int count, const void* rpy, void* R, void* stream) {
  if (count < 0 || !rpy || !R) return fail(MDS_EINVAL, "mds_rpy_to_rot: bad argument");
  if (count == 0) return MDS_OK;
  if (dtype != MDS_F32 && dtype != MDS_F64 && dtype != MDS_F16) return fail(MDS_EINVAL, "mds_rpy_to_rot: dtype");
  with_dtype(dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_rpy_to_rot<T, S><<<grid_for(count, 256), 256, 0, (hipStream_t)stream>>>(count, (const S*)rpy, (S*)R);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_geo_model_to_obs(int dtype, int count, const void* x18, void* obs16, void* stream) {
  if (count < 0 || !x18 || !obs16) return fail(MDS_EINVAL, "mds_geo_model_to_obs: bad argument");
  if (count == 0) return MDS_OK;
  if (dtype != MDS_F32 && dtype != MDS_F64 && dtype != MDS_F16) return fail(MDS_EINVAL, "mds_geo_model_to_obs: dtype");
  with_dtype(dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_geo_model_to_obs<T, S><<<grid_for(count, 256), 256, 0, (hipStream_t)stream>>>(count, (const S*)x18, (S*)obs16);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

#endif  // MDS_PART & 1
#if MDS_PART & 2
int mds_cbf_configure(mds_handle* h, const mds_cbf_params* p, const double* obstacles) {
  MDS_DEV(h);
  if (!h || !p) return fail(MDS_EINVAL, "mds_cbf_configure: null argument");
  if (p->order != 2 && p->order != 3) return fail(MDS_EINVAL, "mds_cbf_configure: order must be 2 or 3");
  if (p->n_obs < 0 || p->n_obs > kCbfMaxObs) return fail(MDS_EINVAL, "mds_cbf_configure: n_obs out of range");
  if (p->n_obs > 0 && !obstacles) return fail(MDS_EINVAL, "mds_cbf_configure: obstacles_host is NULL");
  if (h->cfg.num_drones > kCbfMaxD) return fail(MDS_EUNSUPPORTED, "mds_cbf_configure: more than 32 drones per env");
  if (h->cfg.dtype == MDS_F16) return fail(MDS_EUNSUPPORTED, "mds_cbf_configure: fp16 storage");
  if (!(p->zscale > 0) || !(p->safety_radius > 0)) return fail(MDS_EINVAL, "mds_cbf_configure: zscale / safety_radius");
  const int D = h->cfg.num_drones, npairs = D * (D - 1) / 2;
  const bool new_pairs = !h->pair_ij && npairs > 0;
  std::vector<DevMem::Want> bufs = {{&h->obstacles, sizeof(double) * 4 * kCbfMaxObs},
                                    {&h->cbf_order, sizeof(int) * 9 * (size_t)h->cfg.num_envs},
                                    {&h->cbf_count, sizeof(int) * 12},
                                    {&h->cbf_cost, sizeof(int) * (size_t)h->cfg.num_envs, true}};
  if (new_pairs) bufs.push_back({&h->pair_ij, sizeof(int) * npairs});
  if (int rc = h->mem.alloc_all(bufs)) return rc;
  if (new_pairs) {
    std::vector<int> host(npairs);
    int r = 0;
    for (int i = 0; i < D - 1; ++i)
      for (int j = i + 1; j < D; ++j) host[r++] = i | (j << 8);
    if (hipError_t e = hipMemcpy(h->pair_ij, host.data(), sizeof(int) * npairs, hipMemcpyHostToDevice)) {
      h->mem.release(&h->pair_ij);              // (never a table without its contents: the next call builds it again)
      return fail_hip(e, "mds_cbf_configure: pair table");
    }
  }
  if (p->n_obs > 0) {
    if (h->cfg.dtype == MDS_F64) {
      MDS_HIP(hipMemcpy(h->obstacles, obstacles, sizeof(double) * 4 * p->n_obs, hipMemcpyHostToDevice));
    } else {
      float tmp[4 * kCbfMaxObs];
      for (int k = 0; k < 4 * p->n_obs; ++k) tmp[k] = (float)obstacles[k];
      MDS_HIP(hipMemcpy(h->obstacles, tmp, sizeof(float) * 4 * p->n_obs, hipMemcpyHostToDevice));
    }
  }
  h->cbf_calls = h->cbf_calls_half[0] = h->cbf_calls_half[1] = -1;   // a new problem: forget the cost classes
  {
    const char* solver = getenv("MDS_CBF_SOLVER");
    h->cbf_hildreth = solver && solver[0] == 'h';
    const char* q4e = getenv("MDS_CBF_Q4");
    h->cbf_q4 = q4e && q4e[0] == '1';
    if (const char* fused = getenv("MDS_CBF_FUSED")) h->cbf_fused = fused[0] == '1';       // unset: what mds_cbf_set_step_kernel chose
  }
  h->cbf = *p;
  fill_cbf_params(h->cfg, *p, h->p32.cbf);
  fill_cbf_params(h->cfg, *p, h->p64.cbf);
  h->has_cbf = true;
  return MDS_OK;
}

int mds_cbf_num_rows(const mds_handle* h) {
  if (!h || !h->has_cbf) return fail(MDS_ESTATE, "mds_cbf_num_rows: call mds_cbf_configure first");
  return cbf_num_rows(h->cfg.num_drones, h->cbf.order, h->cbf.n_obs);
}

int mds_cbf_rows(mds_handle* h, const void* x, const void* xdes, void* G, void* hv, void* stream) {
  MDS_DEV(h);
  if (!h || !x || !xdes || !G || !hv) return fail(MDS_EINVAL, "mds_cbf_rows: null argument");
  if (!h->has_cbf) return fail(MDS_ESTATE, "mds_cbf_rows: call mds_cbf_configure first");
  hipStream_t st = (hipStream_t)stream;
  const int E = h->cfg.num_envs;
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {          // the ECBF filter: f32 / f32c / f64 (mds_cbf_configure refuses fp16 storage)
    using T = typename decltype(DT)::T;
    with_int<2, 3>(h->cbf.order, [&](auto ORD) {
      k_cbf_rows<T, T, ORD()><<<E, 256, 0, st>>>(params<T>(h).cbf, E, h->pair_ij, (const T*)h->obstacles, (const T*)x, (const T*)xdes, (T*)G, (T*)hv);
    });
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

static int cbf_filter_range(mds_handle* h, const void* obs_, const void* xdes_, const void* unom_, void* usafe_, int32_t* status_,
                            void* stream, EnvRange rg) {
  hipStream_t st = (hipStream_t)stream;
  const int E = rg.ne, D = h->cfg.num_drones, order = h->cbf.order;
  // an env's blocks are contiguous in every operand: a range is a pointer offset
  const size_t es = elem_size(h->cfg.dtype), d0 = (size_t)rg.e0 * D;
  const char* obs = (const char*)obs_ + d0 * kObsDim * es;
  const char* xdes = (const char*)xdes_ + d0 * (order == 2 ? 9 : 10) * es;
  const char* unom = (const char*)unom_ + d0 * 4 * es;
  char* usafe = (char*)usafe_ + d0 * 4 * es;
  int32_t* status = status_ + rg.e0;
  int& calls = rg.slot == 0 ? h->cbf_calls : h->cbf_calls_half[rg.slot - 1];
  int* const order_tab = h->cbf_order + (size_t)rg.slot * 3 * h->cfg.num_envs;
  int* const count_tab = h->cbf_count + 4 * rg.slot;
  int* const cost_tab = h->cbf_cost + rg.e0;
  const int nv = order == 2 ? 1 : 3, n = nv * D;
  const int m = D * (D - 1) / 2 + D * h->cbf.n_obs + 2 * n;          // rows of the coupled sub-problem
  const int R = (m + 63) / 64;
  const int max_iter = h->cbf.max_iter > 0 ? h->cbf.max_iter : 64 * m;
  const dim3 grid((unsigned)((E + 3) / 4));                // Hildreth kernel: 4 envs per workgroup
  const bool hildreth = h->cbf_hildreth && order == 2;     // MDS_CBF_SOLVER=hildreth at configure time: the coordinate-ascent kernel (A/B)
  if (n > 64) return fail(MDS_EUNSUPPORTED, "mds_cbf_filter: more than 64 coupled QP variables per env");
  if (R > 17) return fail(MDS_EUNSUPPORTED, "mds_cbf_filter: too many rows per env");
  // longest-first dispatch (see k_cbf_filter_gi): classes from the iteration counts of an earlier launch, rebuilt every 8th call
  const int* ord_in = calls < 0 ? nullptr : order_tab;
  const int* cnt_in = calls < 0 ? nullptr : count_tab;
  int* cost_out = hildreth ? nullptr : cost_tab;
  // order 2 with at most 16 thrust variables and 224 rows: four envs per wavefront, one per 16-lane row (k_cbf_filter_q4)
  const bool q4 = h->cbf_q4 && !hildreth && order == 2 && n <= 16 && m <= 224;
  const int RR = R <= 4 ? 4 : (R <= 8 ? 8 : 17);           // row registers per lane the kernels are built for
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {          // f32 / f32c / f64 (mds_cbf_configure refuses fp16 storage)
    using T = typename decltype(DT)::T;
    const CbfParams<T>& P = params<T>(h).cbf;
    const double tol = h->cbf.tol > 0 ? h->cbf.tol : (sizeof(T) == 8 ? 1e-12 : 1e-6);
    const T tol2 = (T)(tol * tol);
    if (q4) {
      with_int<8, 14>(m <= 128 ? 8 : 14, [&](auto RL) {
        k_cbf_filter_q4<T, T, RL()><<<grid, 64, 0, st>>>(P, E, h->pair_ij, (const T*)h->obstacles, (const T*)obs, (const T*)xdes, (const T*)unom,
                                                         (T*)usafe, (int*)status, max_iter, tol2, cost_out);
      });
    } else if (hildreth) {
      with_int<4, 8, 17>(RR, [&](auto R_) {
        k_cbf_filter_o2<T, T, R_()><<<grid, 256, 0, st>>>(P, E, h->pair_ij, (const T*)h->obstacles, (const T*)obs, (const T*)xdes, (const T*)unom,
                                                          (T*)usafe, (int*)status, max_iter, tol2);
      });
    } else {
      // one wavefront (= one env) per workgroup; NMAX bounds the QP variables (LDS footprint of Q, R ~ NMAX^2)
      auto gi = [&](auto ORD, auto NMAX) {
        with_int<4, 8, 17>(RR, [&](auto R_) {
          k_cbf_filter_gi<T, T, R_(), NMAX(), ORD()><<<dim3((unsigned)E), 64, 0, st>>>(P, E, (T)h->cfg.KF, h->pair_ij, (const T*)h->obstacles,
                                                                                      (const T*)obs, (const T*)xdes, (const T*)unom, (T*)usafe,
                                                                                      (int*)status, max_iter, tol2, ord_in, cnt_in, cost_out);
        });
      };
      if (order == 2) with_int<16, 32>(n <= 16 ? 16 : 32, [&](auto NMAX) { gi(std::integral_constant<int, 2>{}, NMAX); });
      else with_int<24, 48, 63>(n <= 24 ? 24 : (n <= 48 ? 48 : 63), [&](auto NMAX) { gi(std::integral_constant<int, 3>{}, NMAX); });
    }
  });
  MDS_HIP(hipGetLastError());
  if (!hildreth && !q4 && E >= 1024) {                    // small batches have no tail to hide
    if (calls < 0 || calls >= 7) {
      k_cbf_order<<<1, kOrderThreads, 0, st>>>(E, cost_tab, order_tab, count_tab);
      MDS_HIP(hipGetLastError());
      calls = 0;
    } else {
      ++calls;
    }
  }
  return MDS_OK;
}

int mds_cbf_filter(mds_handle* h, const void* obs, const void* xdes, const void* unom, void* usafe, int32_t* status,
                   void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !xdes || !unom || !usafe || !status) return fail(MDS_EINVAL, "mds_cbf_filter: null argument");
  if (!h->has_cbf) return fail(MDS_ESTATE, "mds_cbf_filter: call mds_cbf_configure first");
  return cbf_filter_range(h, obs, xdes, unom, usafe, status, stream, EnvRange{0, h->cfg.num_envs, 0});
}

int mds_cbf_last_iterations(mds_handle* h, int32_t* iters_dev, void* stream) {
  MDS_DEV(h);
  if (!h || !iters_dev) return fail(MDS_EINVAL, "mds_cbf_last_iterations: null argument");
  if (!h->has_cbf || !h->cbf_cost) return fail(MDS_ESTATE, "mds_cbf_last_iterations: call mds_cbf_configure first");
  MDS_HIP(hipMemcpyAsync(iters_dev, h->cbf_cost, sizeof(int) * (size_t)h->cfg.num_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MDS_OK;
}

int mds_default_dslpid_gains(mds_dslpid_gains* g) {
  if (!g) return fail(MDS_EINVAL, "mds_default_dslpid_gains");
  const double pf[3] = {.4, .4, 1.25}, ifo[3] = {.05, .05, .05}, df[3] = {.2, .2, .5};
  const double pt[3] = {70000., 70000., 60000.}, it[3] = {.0, .0, 500.}, dt[3] = {20000., 20000., 12000.};
  for (int k = 0; k < 3; ++k) {
    g->P_COEFF_FOR[k] = pf[k]; g->I_COEFF_FOR[k] = ifo[k]; g->D_COEFF_FOR[k] = df[k];
    g->P_COEFF_TOR[k] = pt[k]; g->I_COEFF_TOR[k] = it[k]; g->D_COEFF_TOR[k] = dt[k];
  }
  return MDS_OK;
}

int mds_set_dslpid_gains(mds_handle* h, const mds_dslpid_gains* g) {
  if (!h || !g) return fail(MDS_EINVAL, "mds_set_dslpid_gains: null argument");
  for (int k = 0; k < 3; ++k) {
    DslPidGains<double>& d = h->p64.pid;
    DslPidGains<float>& f = h->p32.pid;
    d.Pf[k] = g->P_COEFF_FOR[k]; d.If[k] = g->I_COEFF_FOR[k]; d.Df[k] = g->D_COEFF_FOR[k];
    d.Pt[k] = g->P_COEFF_TOR[k]; d.It[k] = g->I_COEFF_TOR[k]; d.Dt[k] = g->D_COEFF_TOR[k];
    f.Pf[k] = (float)g->P_COEFF_FOR[k]; f.If[k] = (float)g->I_COEFF_FOR[k]; f.Df[k] = (float)g->D_COEFF_FOR[k];
    f.Pt[k] = (float)g->P_COEFF_TOR[k]; f.It[k] = (float)g->I_COEFF_TOR[k]; f.Dt[k] = (float)g->D_COEFF_TOR[k];
  }
  return MDS_OK;
}

int mds_dslpid_reset(mds_handle* h, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_dslpid_reset: null handle");
  MDS_HIP(hipMemsetAsync(h->pid, 0, 9 * h->ld * comp_size(h->cfg.dtype), (hipStream_t)stream));
  return MDS_OK;
}

// k_dslpid over the batches [batch0, batch0 + nb) (nb == 0: the whole shard).  step: the controller and the physics step of one
// MultiDroneEnv.sim_step (reads the handle's state; obs_in unused); else the controller alone on obs_in (or the handle's state), action to act.
static void launch_dslpid(mds_handle* h, bool step, const void* obs_in, const void* tpos, const void* trpy, void* obs, void* act, hipStream_t st,
                          unsigned batch0 = 0, unsigned nb = 0) {
  const dim3 grid = nb ? dim3(nb) : grid_for(h->n, kBlock);
  auto launch = [&](auto STEP, auto RK4, auto DRAG) {
    with_dtype(h->cfg.dtype, [&](auto DT) {
      using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
      k_dslpid<T, S, STEP(), RK4(), DRAG()><<<grid, kBlock, 0, st>>>(params<T>(h).c, params<T>(h).pid, h->n, h->ld, (T)(1.0 / h->cfg.ctrl_freq),
                                                                   (S*)h->state, (const T*)h->origin, (T*)rpm_track(h), (T*)h->pid, (const S*)obs_in,
                                                                   (const S*)tpos, (const S*)trpy, (S*)obs, (S*)act, (int)batch0, (S*)h->state_lo);
    });
  };
  if (step) with_flags([&](auto RK4, auto DRAG) { launch(std::true_type{}, RK4, DRAG); }, h->cfg.integrator == MDS_INTEGRATOR_RK4, has_drag(h));
  else launch(std::false_type{}, std::false_type{}, std::false_type{});         // the controller alone integrates nothing: one instantiation
}

// One MultiDroneEnv.sim_step of the batches ch covers.  Ground effect / downwash handles (always one chain): the controller reads the
// handle's state and leaves the action in act_scratch (or the caller's buffer), then env.step runs it one substep per launch.
static int step_dslpid(mds_handle* h, const void* tpos, const void* trpy, void* obs, void* act, const Chain& ch) {
  if (h->envfx) {
    if (!act) act = h->act_scratch;
    launch_dslpid(h, false, nullptr, tpos, trpy, nullptr, act, ch.st);
    return step_env_plain(h, act, obs, ch.st, 0);
  }
  launch_dslpid(h, true, nullptr, tpos, trpy, obs, act, ch.st, ch.i0, ch.n);
  return MDS_OK;
}

int mds_dslpid_compute(mds_handle* h, const void* obs_in, const void* tpos, const void* trpy, void* act, void* stream) {
  MDS_DEV(h);
  if (!h || !obs_in || !tpos || !trpy || !act) return fail(MDS_EINVAL, "mds_dslpid_compute: null argument");
  if (!aligned16(act)) return fail(MDS_EALIGN, "mds_dslpid_compute: rpm_dev");
  launch_dslpid(h, false, obs_in, tpos, trpy, nullptr, act, (hipStream_t)stream);
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_step_dslpid(mds_handle* h, const void* tpos, const void* trpy, void* obs, void* act, void* stream) {
  MDS_DEV(h);
  if (!h || !tpos || !trpy) return fail(MDS_EINVAL, "mds_step_dslpid: null argument");
  if (!aligned16(obs) || !aligned16(act)) return fail(MDS_EALIGN, "mds_step_dslpid: obs_dev/action_dev");
  if (int rc = step_dslpid(h, tpos, trpy, obs, act, Chain{(hipStream_t)stream, 0, 0})) return rc;
  return check_launches();
}

int mds_rollout_dslpid(mds_handle* h, const void* tpos, const void* trpy, int n_target_sets, int first_step, int n_steps, void* obs,
                       int obs_every_step, void* stream) {
  MDS_DEV(h);
  if (!h || !tpos || !trpy || n_target_sets < 1 || first_step < 0 || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_dslpid: arguments");
  if (!aligned16(obs)) return fail(MDS_EALIGN, "mds_rollout_dslpid: obs_dev");
  const size_t set_bytes = (size_t)h->n * 3 * elem_size(h->cfg.dtype);
  // the PID memory is per drone too: the two halves of a big shard are two independent chains, as in mds_rollout_geometric
  auto step = [&](int k, const Chain* ch, int nc) -> int {
    const size_t off = (size_t)(((long long)first_step + k) % n_target_sets) * set_bytes;
    void* o = (obs_every_step || k == n_steps - 1) ? obs : nullptr;
    for (int c = 0; c < nc; ++c)
      if (int rc = step_dslpid(h, (const char*)tpos + off, (const char*)trpy + off, o, nullptr, ch[c])) return rc;
    return MDS_OK;
  };
  return step_loop_batches(h, (hipStream_t)stream, 0, n_steps, step);
}

int mds_set_lqr_omega_gain(mds_handle* h, const double K[36]) {
  MDS_DEV(h);
  if (!h || !K) return fail(MDS_EINVAL, "mds_set_lqr_omega_gain: null argument");
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 9; ++k) {
      h->p64.lqr.k[r][k] = K[9 * r + k];
      h->p32.lqr.k[r][k] = (float)K[9 * r + k];
    }
  h->has_lqr = true;
  return upload_gain(h, 1, h->p32.lqr, h->p64.lqr);
}

int mds_lqr_omega_compute(mds_handle* h, const void* obs, const void* des, void* u, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !des || !u) return fail(MDS_EINVAL, "mds_lqr_omega_compute: null argument");
  if (!h->has_lqr) return fail(MDS_ESTATE, "mds_lqr_omega_compute: call mds_set_lqr_omega_gain first");
  if (!aligned16(u)) return fail(MDS_EALIGN, "mds_lqr_omega_compute: u_dev");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_lqr_omega_compute<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(params<T>(h).c, params<T>(h).lqr, h->n, (const S*)obs, (const S*)des, (S*)u);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_set_lqr_gain(mds_handle* h, const double K[48]) {
  MDS_DEV(h);
  if (!h || !K) return fail(MDS_EINVAL, "mds_set_lqr_gain: null argument");
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 12; ++k) {
      h->p64.lqr12.k[r][k] = K[12 * r + k];
      h->p32.lqr12.k[r][k] = (float)K[12 * r + k];
    }
  h->has_lqr12 = true;
  return upload_gain(h, 0, h->p32.lqr12, h->p64.lqr12);
}

int mds_lqr_compute(mds_handle* h, const void* obs, const void* des, void* u, void* action, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !des || (!u && !action)) return fail(MDS_EINVAL, "mds_lqr_compute: null argument");
  if (!h->has_lqr12) return fail(MDS_ESTATE, "mds_lqr_compute: call mds_set_lqr_gain first");
  if (!aligned16(u) || !aligned16(action)) return fail(MDS_EALIGN, "mds_lqr_compute: u_dev/action_dev");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_lqr12_compute<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(params<T>(h).c, params<T>(h).lqr12, h->n, (const S*)obs, (const S*)des, (S*)u,
                                                                (S*)action);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

// one control step of the 12-state LQR (trajectory sample -> LQRController -> env.step) on the whole shard
int step_lqr(mds_handle* h, double t, void* obs, void* act, hipStream_t st) {
  if (h->envfx) return step_env_ctrl(h, 1, t, nullptr, 0.0, obs, act, st);
  const dim3 grid = grid_for(h->n, kBlock);
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  with_flags([&](auto RK4, auto DRAG) {
    with_dtype(h->cfg.dtype, [&](auto DT) {
      using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
      k_step_lqr<T, S, RK4(), DRAG()><<<grid, kBlock, 0, st>>>(params<T>(h).c, params<T>(h).lqr12, h->n, h->ld, t, h->traj_mode, (S*)h->state,
                                                               (const T*)h->origin, (const T*)h->lem, SegTable{h->segs, h->nseg_total}, h->tinfo,
                                                               (T*)rpm_track(h), (S*)obs, (S*)act, (S*)h->state_lo);
    });
  }, rk4, drag);
  return MDS_OK;
}

int mds_step_lqr(mds_handle* h, double t, void* obs, void* act, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_step_lqr: null handle");
  if (!h->has_traj) return fail(MDS_ESTATE, "mds_step_lqr: call mds_set_lemniscate / mds_set_trajectory_segments first");
  if (!h->has_lqr12) return fail(MDS_ESTATE, "mds_step_lqr: call mds_set_lqr_gain first");
  if (!aligned16(obs) || !aligned16(act)) return fail(MDS_EALIGN, "mds_step_lqr: obs_dev/action_dev");
  if (int rc = step_lqr(h, t, obs, act, (hipStream_t)stream)) return rc;
  return check_launches();
}

int mds_set_lqr_yank_omega_gain(mds_handle* h, const double K[40]) {
  MDS_DEV(h);
  if (!h || !K) return fail(MDS_EINVAL, "mds_set_lqr_yank_omega_gain: null argument");
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 10; ++k) {
      h->p64.lqr_yo.k[r][k] = K[10 * r + k];
      h->p32.lqr_yo.k[r][k] = (float)K[10 * r + k];
    }
  h->has_lqr_yo = true;
  return upload_gain(h, 2, h->p32.lqr_yo, h->p64.lqr_yo);
}

int mds_lqr_yank_omega_compute(mds_handle* h, const void* obs, const void* des, void* u, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !des || !u) return fail(MDS_EINVAL, "mds_lqr_yank_omega_compute: null argument");
  if (!h->has_lqr_yo) return fail(MDS_ESTATE, "mds_lqr_yank_omega_compute: call mds_set_lqr_yank_omega_gain first");
  if (!aligned16(u)) return fail(MDS_EALIGN, "mds_lqr_yank_omega_compute: u_dev");
  hipStream_t st = (hipStream_t)stream;
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_lqr_yank_omega_compute<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(params<T>(h).c, params<T>(h).lqr_yo, h->n, (const S*)obs, (const S*)des,
                                                                         (S*)u);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_cbf_set_nominal(mds_handle* h, int which) {
  if (!h || which < 0 || which > 3) return fail(MDS_EINVAL, "mds_cbf_set_nominal");
  if (which == 1 && !h->has_lqr) return fail(MDS_ESTATE, "mds_cbf_set_nominal: call mds_set_lqr_omega_gain first");
  if (which == 2 && !h->has_lqr_yo) return fail(MDS_ESTATE, "mds_cbf_set_nominal: call mds_set_lqr_yank_omega_gain first");
  if (which == 3 && !h->dlqr_omega_K)
    return fail(MDS_ESTATE, "mds_cbf_set_nominal: call mds_set_dlqr_omega_gain / mds_dlqr_omega_solve_gain first");
  h->cbf_nominal = which;
  return MDS_OK;
}

int mds_cbf_set_step_kernel(mds_handle* h, int one_launch) {
  if (!h || one_launch < 0 || one_launch > 2) return fail(MDS_EINVAL, "mds_cbf_set_step_kernel");
  h->cbf_fused = one_launch == 1;
  h->cbf_step_persistent = one_launch == 2;
  for (int k = 0; k < 3; ++k) h->next_nom_ok[k] = false;
  return MDS_OK;
}

int mds_cbf_get_step_inputs(mds_handle* h, void* unom, void* usafe, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_cbf_get_step_inputs: null handle");
  if (!h->cbf_unom || h->cbf_last_step_kernel != 0)
    return fail(MDS_ESTATE, "mds_cbf_get_step_inputs: the last filtered step was not issued as QP launch + low-level launch");
  const size_t bytes = (size_t)h->n * 4 * elem_size(h->cfg.dtype);
  if (unom) MDS_HIP(hipMemcpyAsync(unom, h->cbf_unom, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (usafe) MDS_HIP(hipMemcpyAsync(usafe, h->cbf_usafe, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MDS_OK;
}

int mds_cbf_last_step_kernel(const mds_handle* h) {
  if (!h) return fail(MDS_EINVAL, "mds_cbf_last_step_kernel: null handle");
  return h->cbf_last_step_kernel;
}

int mds_lowlevel_reset(mds_handle* h, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_lowlevel_reset: null handle");
  MDS_HIP(hipMemsetAsync(h->ll, 0, 6 * h->ld * comp_size(h->cfg.dtype), (hipStream_t)stream));
  return MDS_OK;
}

static void launch_thrust_omega(mds_handle* h, const void* u, const void* src, int rates_given, int yank, void* rpm, hipStream_t st) {
  with_dtype(h->cfg.dtype, [&](auto DT) {
    using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
    k_thrust_omega<T, S><<<grid_for(h->n, 256), 256, 0, st>>>(params<T>(h).c, h->n, h->ld, (T)(1.0 / h->cfg.ctrl_freq), rates_given, yank, (T*)h->ll,
                                                               (const S*)u, (const S*)src, (S*)rpm);
  });
}

int mds_yank_omega_compute(mds_handle* h, const void* u, const void* obs, void* rpm, void* stream) {
  MDS_DEV(h);
  if (!h || !u || !obs || !rpm) return fail(MDS_EINVAL, "mds_yank_omega_compute: null argument");
  if (!aligned16(u) || !aligned16(rpm)) return fail(MDS_EALIGN, "mds_yank_omega_compute");
  launch_thrust_omega(h, u, obs, 0, 1, rpm, (hipStream_t)stream);
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_thrust_omega_compute(mds_handle* h, const void* u, const void* obs, void* rpm, void* stream) {
  MDS_DEV(h);
  if (!h || !u || !obs || !rpm) return fail(MDS_EINVAL, "mds_thrust_omega_compute: null argument");
  if (!aligned16(u) || !aligned16(rpm)) return fail(MDS_EALIGN, "mds_thrust_omega_compute");
  launch_thrust_omega(h, u, obs, 0, 0, rpm, (hipStream_t)stream);
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_thrust_omega_from_rates(mds_handle* h, const void* u, const void* rates, void* rpm, void* stream) {
  MDS_DEV(h);
  if (!h || !u || !rates || !rpm) return fail(MDS_EINVAL, "mds_thrust_omega_from_rates: null argument");
  if (!aligned16(u) || !aligned16(rpm)) return fail(MDS_EALIGN, "mds_thrust_omega_from_rates");
  launch_thrust_omega(h, u, rates, 1, 0, rpm, (hipStream_t)stream);
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

// nominal controller -> [ECBF QP] -> low level -> env.step.  with_filter = false: the plain loops of
// simulations/EnvGeometricOmega.py / EnvGeometricYankOmega.py (ctrl[j].compute(obs[j]) = LQR + low level, :314 / :319).
// The C rollout loops chain the nominal input from step to step (NominalStep: have_nominal / want_next).
int step_nominal_lowlevel(mds_handle* h, double t, void* obs, int32_t* status, void* action, hipStream_t st, const NominalStep& o) {
  EnvRange rg = o.range;
  const bool with_filter = o.with_filter;
  if (!h->has_traj || h->traj_mode != 1) return fail(MDS_ESTATE, "mds_step_cbf_geometric / mds_step_nominal: call mds_set_lemniscate first");
  if (!aligned16(obs) || !aligned16(action)) return fail(MDS_EALIGN, "mds_step_cbf_geometric / mds_step_nominal: obs_dev/action_dev");
  const bool yank = h->cbf_nominal == 2;
  const size_t es = elem_size(h->cfg.dtype);
  // One-launch form (k_cbf_step): order 2, whole envs per wave (D | 64, D <= 16), explicit Euler without drag, nominal 0 / 1, no
  // action output.  Everything else takes the three launches below.
  {
    const int D = h->cfg.num_drones;
    const int m2 = D * (D - 1) / 2 + D * h->cbf.n_obs + 2 * D;
    if (rg.ne < 0) rg.ne = h->cfg.num_envs;
    const size_t j0 = (size_t)rg.e0 * D, j1 = j0 + (size_t)rg.ne * D;
    if (with_filter && h->cbf_fused && !action && h->cbf.order == 2 && !h->cbf_hildreth && D <= 16 && 64 % D == 0 && m2 <= 512 && !h->envfx &&
        h->cfg.integrator == MDS_INTEGRATOR_EULER && !has_drag(h) && h->cbf_nominal <= 1 && j0 % 64 == 0 && h->cfg.dtype != MDS_F16) {
      const dim3 grid64((unsigned)((j1 - j0 + 63) / 64));
      const int batch0 = (int)(j0 / 64), max_iter = h->cbf.max_iter > 0 ? h->cbf.max_iter : 64 * m2;
      h->cbf_last_step_kernel = 1;
      const void* gain = h->cbf_nominal == 1 ? h->gain_dev[1] : nullptr;
      void* rpm = rpm_track(h);
      with_dtype_no_half(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T;
        const double tol = h->cbf.tol > 0 ? h->cbf.tol : (sizeof(T) == 8 ? 1e-12 : 1e-6);
        with_int<4, 8>(m2 <= 256 ? 4 : 8, [&](auto RR) {
          with_int<1, 0>(h->cbf_nominal, [&](auto NOM) {
            k_cbf_step<T, RR(), NOM(), DT.COMP><<<grid64, 64, 0, st>>>(params<T>(h).c, params<T>(h).cbf, gain, (int)j1, h->ld, h->cfg.num_envs, t,
                                                                       (T)(1.0 / h->cfg.ctrl_freq), (T*)h->state, (T*)h->state_lo, (const T*)h->lem,
                                                                       (T*)rpm, (T*)h->ll, h->pair_ij, (const T*)h->obstacles, (T*)obs, (int*)status,
                                                                       h->cbf_cost, max_iter, (T)(tol * tol), batch0);
          });
        });
      });
      MDS_HIP(hipGetLastError());
      return MDS_OK;
    }
  }
  if (with_filter) h->cbf_last_step_kernel = 0;
  if (!h->cbf_unom)            // (first step only: all three or none, so that cbf_unom alone says "the scratch exists")
    if (int rc = h->mem.alloc_all({{&h->cbf_unom, (size_t)h->n * 4 * es}, {&h->cbf_xdes, (size_t)h->n * 10 * es}, {&h->cbf_usafe, (size_t)h->n * 4 * es}}))
      return rc;
  // drones of the env range: whole 256-drone batches (the caller of a partial range guarantees the alignment)
  if (rg.ne < 0) rg.ne = h->cfg.num_envs;
  const size_t i0 = (size_t)rg.e0 * h->cfg.num_drones, i1 = i0 + (size_t)rg.ne * h->cfg.num_drones;
  const int batch0 = (int)(i0 / kBlock), n_end = (int)i1;
  const dim3 grid = grid_for(i1 - i0, kBlock);
  // the hover force is subtracted from the nominal input only on the way into the filter (CBFTest.py:339, CBFTestOrd3.py:341)
  const double hover_sub = with_filter ? h->cfg.M * h->cfg.G : 0.0;
  const bool skip_nominal = o.have_nominal && h->next_nom_ok[rg.slot] && h->next_nom_t[rg.slot] == t;
  h->next_nom_ok[rg.slot] = false;
  const bool rk4 = h->cfg.integrator == MDS_INTEGRATOR_RK4, drag = has_drag(h);
  const void* nom_K = h->cbf_nominal == 1 ? h->gain_dev[1] : nullptr;
  // k_lowlevel_step: (a) `only` mode = the nominal controller of this step (GeometricControl / LQR-omega: the ONE compiled copy of
  // cbf_nominal_of, see there); (b) low level + physics + observation, optionally followed by the nominal input of the next step
  auto lowlevel = [&](bool yank_ll, const void* u_in, double offs, bool next_on, double t_nx, int only) {
    with_flags([&](auto YANK, auto RK4, auto DRAG) {
      with_dtype(h->cfg.dtype, [&](auto DT) {
        using T = typename decltype(DT)::T; using S = typename decltype(DT)::S;
        const NextNominal<T, S> nx{next_on ? (const T*)h->lem : nullptr, nom_K, next_on ? (S*)h->cbf_unom : nullptr, (S*)h->cbf_xdes, t_nx, (T)hover_sub,
                                   h->cbf_nominal, only};
        k_lowlevel_step<T, S, RK4(), DRAG(), YANK(), DT.COMP><<<grid, kBlock, 0, st>>>(params<T>(h).c, n_end, h->ld, (T)(1.0 / h->cfg.ctrl_freq), (T)offs,
                                                                                      (S*)h->state, (const T*)h->origin, (T*)rpm_track(h), (T*)h->ll,
                                                                                      (const S*)u_in, (S*)obs, (S*)action, batch0, (S*)h->state_lo, nx);
      });
    }, yank_ll, rk4, drag);
  };
  if (skip_nominal) {
    // u_hat / xdes of this step came out of the previous step's low-level launch
  } else if (h->cbf_nominal == 2) {
    with_dtype_no_half(h->cfg.dtype, [&](auto DT) {       // the LQR family: f32 / f32c / f64 only (the entry points refuse fp16 storage)
      using T = typename decltype(DT)::T;
      k_cbf_nominal_lqr_yo<T, T><<<grid, kBlock, 0, st>>>(params<T>(h).c, params<T>(h).lqr_yo, n_end, h->ld, t, (T)hover_sub, (const T*)h->state,
                                                          (const T*)h->lem, (const T*)obs, (T*)h->cbf_unom, (T*)h->cbf_xdes, batch0);
    });
  } else if (h->cbf_nominal == 3) {
    // the coupled dLQR: whole envs per workgroup (k_dlqr_omega_rollout's layout), the env range of this chain
    const int D = h->cfg.num_drones, epb = kFedceBlock / D;
    const dim3 grid_e((unsigned)((rg.ne + epb - 1) / epb));
    with_dtype_no_half(h->cfg.dtype, [&](auto DT) {       // f32 / f64 (mds_set_dlqr_omega_gain refuses the rest)
      using T = typename decltype(DT)::T;
      k_cbf_nominal_dlqr_omega<T, T><<<grid_e, kFedceBlock, 0, st>>>(params<T>(h).c, (const T*)h->dlqr_omega_K, rg.e0, rg.e0 + rg.ne, D, h->ld, t,
                                                                     (T)hover_sub, (const T*)h->state, (const T*)h->lem, (T*)h->cbf_unom,
                                                                     (T*)h->cbf_xdes);
    });
  } else {
    lowlevel(false, nullptr, 0.0, true, t, 1);
  }
  MDS_HIP(hipGetLastError());
  const void* u_ll = h->cbf_unom;
  if (with_filter) {
    int rc = cbf_filter_range(h, obs, h->cbf_xdes, h->cbf_unom, h->cbf_usafe, status, st, rg);
    if (rc != MDS_OK) return rc;
    u_ll = h->cbf_usafe;
  }
  // order 2: u_safe[0] += M G (CBFTest.py:346); order 3: the yank goes to the low level as it is (CBFTestOrd3.py:350)
  const double ll_offset = (with_filter && !yank) ? h->cfg.M * h->cfg.G : 0.0;
  if (h->envfx)            // ground effect / downwash: low level + first substep, then the remaining substeps (whole batch, one stream)
    return step_env_ctrl(h, yank ? 3 : 2, t, u_ll, ll_offset, obs, action, st);
  const bool next_on = o.want_next && !yank && h->cbf_nominal <= 1 && !action;
  h->next_nom_ok[rg.slot] = next_on;
  h->next_nom_t[rg.slot] = o.t_next;
  lowlevel(yank, u_ll, ll_offset, next_on, o.t_next, 0);
  return check_launches();
}

// what k_cbf_rollout covers (mds_rollout_cbf_geometric_fused; mds_cbf_set_step_kernel(h, 2))
static bool roll_fused_applies(const mds_handle* h) {
  const int D = h->cfg.num_drones;
  const int m2 = D * (D - 1) / 2 + 2 * D;                      // pair rows and two bound rows per drone (obstacles are per-drone bounds)
  return h->has_cbf && h->cbf.order == 2 && !h->cbf_hildreth && D >= 1 && D <= 16 && m2 <= 256 && !h->envfx &&
         h->cfg.integrator == MDS_INTEGRATOR_EULER && !has_drag(h) && h->cbf_nominal <= 1 && h->cfg.dtype != MDS_F16 &&
         h->cfg.pyb_freq == h->cfg.ctrl_freq && h->n <= (1 << 27);
}

int mds_step_cbf_geometric(mds_handle* h, double t, void* obs, int32_t* status, void* action, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !status) return fail(MDS_EINVAL, "mds_step_cbf_geometric: null argument");
  if (!h->has_cbf) return fail(MDS_ESTATE, "mds_step_cbf_geometric: call mds_cbf_configure first");
  const bool ord3 = h->cbf.order == 3;
  // the order-3 rows act on (yank, w): only the yank-omega LQR produces that input (simulations/CBFTestOrd3.py:294-297;
  // GeometricControl.compute has no skip_low_level there), and it is meaningless for the order-2 rows
  if (ord3 != (h->cbf_nominal == 2))
    return fail(MDS_EUNSUPPORTED, "mds_step_cbf_geometric: order 3 needs (and order 2 excludes) the lqr-yank-omega nominal, mds_cbf_set_nominal(h, 2)");
  if (h->cfg.dtype == MDS_F16) return fail(MDS_EUNSUPPORTED, "mds_step_cbf_geometric: fp16 storage");
  if (h->cbf_step_persistent && !action && roll_fused_applies(h)) {   // mds_cbf_set_step_kernel(h, 2): one launch of k_cbf_rollout, one step
    for (int k = 0; k < 3; ++k) h->next_nom_ok[k] = false;
    return mds_rollout_cbf_geometric_fused(h, t, 1, 1, nullptr, 0, 0, obs, status, nullptr, stream);
  }
  NominalStep o;
  o.with_filter = true;
  return step_nominal_lowlevel(h, t, obs, status, action, (hipStream_t)stream, o);
}

int mds_rollout_cbf_geometric(mds_handle* h, double t0, int n_steps, void* obs, int32_t* status, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !status || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_cbf_geometric: null argument");
  if (h->cbf_step_persistent && h->has_cbf && h->cbf.order == 2 && h->cbf_nominal <= 1 && roll_fused_applies(h) && h->has_traj && h->traj_mode == 1) {
    for (int k = 0; k < 3; ++k) h->next_nom_ok[k] = false;
    h->last_rollout_streams = 1;
    return mds_rollout_cbf_geometric_fused(h, t0, n_steps, 25, nullptr, 0, 0, obs, status, nullptr, stream);
  }
  // The env halves are independent step chains (a barrier row couples drones of one env only).  On two streams one half's
  // QP kernel (latency / ALU bound) runs beside the other half's nominal and low-level kernels (memory bound).  The split
  // must fall on a 256-drone batch boundary; each half keeps its own cost classes for the longest-first dispatch.
  const int E = h->cfg.num_envs, D = h->cfg.num_drones;
  int e_mid = 0;
  for (int e = E / 2; e > 0 && e >= E / 2 - 256; --e)
    if (((size_t)e * D) % kBlock == 0) {
      e_mid = e;
      break;
    }
  const double dt = 1.0 / h->cfg.ctrl_freq;
  double t = t0;
  if (n_steps > 0) {     // validation and scratch allocation: the first step is a plain one, whole batch, on the caller's stream
    if (int rc = mds_step_cbf_geometric(h, t, obs, status, nullptr, stream)) return rc;
    t += dt;
  }
  auto step = [&](int k, const Chain* ch, int nc) -> int {
    // each chain's low-level launch of step k also computes the nominal input of its step k + 1 (next_nominal), so that
    // from its second step on a chain is two launches per step: QP, low level
    NominalStep o;
    o.with_filter = true; o.have_nominal = k > 1; o.want_next = k < n_steps - 1; o.t_next = t + dt;
    for (int c = 0; c < nc; ++c) {
      o.range = ch[c].n ? EnvRange{(int)ch[c].i0, (int)ch[c].n, c + 1} : EnvRange{0, E, 0};
      if (int rc = step_nominal_lowlevel(h, t, obs, status, nullptr, ch[c].st, o)) return rc;
    }
    t += dt;
    return MDS_OK;
  };
  return step_loop(h, (hipStream_t)stream, rollout_streams_policy(h, 1, n_steps), (unsigned)e_mid, (unsigned)E, 1, n_steps, step);
}

int mds_rollout_cbf_geometric_fused(mds_handle* h, double t0, int n_steps, int steps_per_launch, void* obs_log, int log_slots, int first_slot,
                                    void* obs, int32_t* status, int32_t* status_log, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !status || n_steps < 0 || steps_per_launch < 1 || log_slots < 0 || first_slot < 0 || (obs_log && first_slot >= log_slots) ||
      (obs_log && log_slots < 1))
    return fail(MDS_EINVAL, "mds_rollout_cbf_geometric_fused: null or out-of-range argument");
  if (!h->has_cbf) return fail(MDS_ESTATE, "mds_rollout_cbf_geometric_fused: call mds_cbf_configure first");
  if (!h->has_traj || h->traj_mode != 1) return fail(MDS_ESTATE, "mds_rollout_cbf_geometric_fused: call mds_set_lemniscate first");
  if (!aligned16(obs) || !aligned16(obs_log)) return fail(MDS_EALIGN, "mds_rollout_cbf_geometric_fused: obs buffers");
  const int D = h->cfg.num_drones;
  const int m2 = D * (D - 1) / 2 + D * h->cbf.n_obs + 2 * D;
  if (h->cbf_nominal == 3)
    return fail(MDS_EUNSUPPORTED, "mds_rollout_cbf_geometric_fused: the dlqr-omega nominal couples the drones of an env and is served by "
                                  "mds_step_cbf_geometric / mds_rollout_cbf_geometric only");
  if (h->cbf.order == 3) {
    // the order-3 loop (simulations/CBFTestOrd3.py:306-352): k_cbf_rollout_o3, one wavefront per env, steps_per_launch steps per launch
    if (!(h->cbf_nominal == 2 && h->has_lqr_yo && D <= 16 && !h->envfx && !h->cbf_hildreth && h->cfg.integrator == MDS_INTEGRATOR_EULER && !has_drag(h) &&
          (h->cfg.dtype == MDS_F32 || h->cfg.dtype == MDS_F64) && h->cfg.pyb_freq == h->cfg.ctrl_freq))
      return fail(MDS_EUNSUPPORTED, "mds_rollout_cbf_geometric_fused (order 3): lqr-yank-omega nominal, D <= 16, explicit Euler at pyb_freq == ctrl_freq "
                                    "without drag / ground effect / downwash, f32 / f64");
    if (n_steps == 0) return MDS_OK;
    hipStream_t st3 = (hipStream_t)stream;
    const int m3 = D * (D - 1) / 2 + D * h->cbf.n_obs + 6 * D, n3 = 3 * D;
    const int max_iter3 = h->cbf.max_iter > 0 ? h->cbf.max_iter : 64 * m3;
    const double dt3 = 1.0 / h->cfg.ctrl_freq, hover_sub = h->cfg.M * h->cfg.G;      // the hover force is subtracted from the yank on the way into the filter (:341)
    void* rpm3 = rpm_track(h);
    h->cbf_last_step_kernel = 2;
    for (Chunks c{n_steps, steps_per_launch, t0, dt3, first_slot, obs_log ? log_slots : 0}; c.k < n_steps; c.advance(c.len())) {
      const int ks = c.len(), slot3 = c.slot;
      const double t3 = c.t;
      int32_t* slog = status_log ? status_log + (size_t)c.k * h->cfg.num_envs : nullptr;
      with_dtype_no_half(h->cfg.dtype, [&](auto DT) {       // f32 / f64 (checked above)
        using T = typename decltype(DT)::T;
        const double tol = h->cbf.tol > 0 ? h->cbf.tol : (sizeof(T) == 8 ? 1e-12 : 1e-6);
        auto launch = [&](auto RR, auto NM) {               // row registers per lane, bound on the QP variables
          k_cbf_rollout_o3<T, RR(), NM()><<<dim3((unsigned)h->cfg.num_envs), 64, 0, st3>>>(
              params<T>(h).c, params<T>(h).cbf, params<T>(h).lqr_yo, h->cfg.num_envs, h->ld, t3, dt3, ks, (T*)h->state, (const T*)h->lem, (T*)rpm3,
              (T*)h->ll, h->pair_ij, (const T*)h->obstacles, (T*)obs, (T*)obs_log, slot3, log_slots > 0 ? log_slots : 1, (int*)status, (int*)slog,
              h->cbf_cost, max_iter3, (T)(tol * tol), (T)hover_sub);
        };
        if (n3 <= 24 && m3 <= 256) launch(std::integral_constant<int, 4>{}, std::integral_constant<int, 24>{});
        else launch(std::integral_constant<int, 8>{}, std::integral_constant<int, 48>{});
      });
      MDS_HIP(hipGetLastError());
    }
    return MDS_OK;
  }
  // what the persistent kernel covers (everything else: mds_rollout_cbf_geometric, one or two launches per step)
  if (!roll_fused_applies(h))
    return fail(MDS_EUNSUPPORTED, "mds_rollout_cbf_geometric_fused: order-2 CBF, D <= 16, explicit Euler at "
                                  "pyb_freq == ctrl_freq without drag / ground effect / downwash, geometric or LQR-omega nominal, f32 / f32c / f64, "
                                  "at most 2^27 drones (32-bit byte offsets into the per-drone planes)");
  if (n_steps == 0) return MDS_OK;
  hipStream_t st = (hipStream_t)stream;
  // wavefronts per workgroup: 8 in fp32 (two workgroups per CU at <= 128 VGPRs); 4 in double (one wavefront per SIMD: the double
  // instantiation needs more than the 256 registers two wavefronts per SIMD would leave it)
  constexpr int NWF = 8, NWD = 4;
  const int nw = h->cfg.dtype == MDS_F64 ? NWD : NWF;
  // a workgroup owns 64 nw / Dp whole envs, Dp = the env width padded to 4, 8 or 16 lanes (any D <= 16)
  const int Dp = D <= 4 ? 4 : (D <= 8 ? 8 : 16), envs_per_wg = 64 * nw / Dp;
  const dim3 grid((unsigned)((h->cfg.num_envs + envs_per_wg - 1) / envs_per_wg));
  const int max_iter = h->cbf.max_iter > 0 ? h->cbf.max_iter : 64 * m2;
  const void* gain = h->cbf_nominal == 1 ? h->gain_dev[1] : nullptr;
  const double dt = 1.0 / h->cfg.ctrl_freq;
  void* rpm = rpm_track(h);
  const size_t es = elem_size(h->cfg.dtype);
  h->cbf_last_step_kernel = 2;
  // tuning aid: MDS_TUNE_ROLL_STAMPS=1 -> per-wave shader-clock ticks by part of the step, summed over this call, printed to stderr
  // (synchronises the stream: never set it in production)
  unsigned long long* stamps_base = nullptr;
  DevMem stamps_mem(kHipAllocator);             // the call's own temporary, not the handle's: freed on every way out of this function
  const size_t n_stamp = (size_t)grid.x * nw * 10;
  if (const char* e = getenv("MDS_TUNE_ROLL_STAMPS"))
    if (e[0] == '1')
      if (int rc = stamps_mem.alloc(&stamps_base, n_stamp * sizeof(unsigned long long) * ((n_steps + steps_per_launch - 1) / steps_per_launch)))
        return rc;
  unsigned long long* stamps_dev = stamps_base;
  // (t advances on the host exactly as inside the kernel, one += per step, so that consecutive launches continue the same sequence)
  for (Chunks c{n_steps, steps_per_launch, t0, dt, first_slot, obs_log ? log_slots : 0}; c.k < n_steps; c.advance(c.len())) {
    const int ks = c.len(), slot = c.slot;
    const double t = c.t;
    int32_t* slog = status_log ? status_log + (size_t)c.k * h->cfg.num_envs : nullptr;
    with_dtype_no_half(h->cfg.dtype, [&](auto DT) {         // f32 / f32c / f64 (roll_fused_applies)
      using T = typename decltype(DT)::T;
      const double tol = h->cbf.tol > 0 ? h->cbf.tol : (sizeof(T) == 8 ? 1e-12 : 1e-6);
      RollArgs<T> ra;
      ra.p.c = params<T>(h).c; ra.p.P = params<T>(h).cbf; ra.Kp = gain; ra.n = (int)h->n; ra.ld = h->ld; ra.E = h->cfg.num_envs;
      ra.t = t; ra.ctrl_dt = dt; ra.n_steps = ks; ra.state = (T*)h->state; ra.state_lo = (T*)h->state_lo; ra.lem = (const T*)h->lem;
      ra.last_rpm = (T*)rpm; ra.ll = (T*)h->ll; ra.pair_ij = h->pair_ij; ra.obstacles = (const T*)h->obstacles; ra.obs_log = (T*)obs_log;
      ra.slot = slot; ra.n_slots = log_slots > 0 ? log_slots : 1; ra.obs_last = (T*)obs; ra.status = (int*)status; ra.status_log = (int*)slog;
      ra.cost_io = h->cbf_cost; ra.max_iter = max_iter; ra.tol2 = (T)(tol * tol); ra.tol = (T)tol; ra.stamps = stamps_dev;
      with_int<1, 0>(h->cbf_nominal, [&](auto NOM) {
        with_flags([&](auto PAD) {                          // PAD: the env width D is not itself 4, 8 or 16 lanes
          k_cbf_rollout<T, NOM(), DT.COMP, (sizeof(T) == 8 ? NWD : NWF), PAD()><<<grid, 64 * nw, 0, st>>>(ra);
        }, D != Dp);
      });
    });
    MDS_HIP(hipGetLastError());
    if (stamps_dev) stamps_dev += n_stamp;
  }
  if (stamps_base) {
    const int launches = (n_steps + steps_per_launch - 1) / steps_per_launch;
    std::vector<unsigned long long> hs(n_stamp * launches);
    MDS_HIP(hipStreamSynchronize(st));
    MDS_HIP(hipMemcpy(hs.data(), stamps_base, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    static const char* part[10] = {"wait before B", "stage B", "wait after B", "stage C", "obs rows", "stage A", " B: ticket", " B: rows", " B: bookkeeping", " B: scan+solve"};
    const size_t waves = (size_t)grid.x * nw;
    double tot_mean = 0;
    for (int p = 0; p < 10; ++p) {
      double sum = 0, mx = 0;
      for (size_t w = 0; w < waves; ++w) {
        double v = 0;
        for (int l = 0; l < launches; ++l) v += (double)hs[(size_t)l * n_stamp + w * 10 + p];
        sum += v;
        if (v > mx) mx = v;
      }
      if (p < 6) tot_mean += sum / waves / n_steps;
      fprintf(stderr, "[mds roll stamps] %-14s mean %9.0f  max %9.0f ticks per wave and step\n", part[p], sum / waves / n_steps, mx / n_steps);
    }
    fprintf(stderr, "[mds roll stamps] total mean %.0f ticks per wave and step, %d steps, %zu waves\n", tot_mean, n_steps, waves);
  }
  if (obs_log) {       // the kernel materialises each step's observation once, in its log slot: obs_dev gets a copy of the last one
    const size_t row = (size_t)h->n * kObsDim * es;
    const int last = (first_slot + n_steps - 1) % log_slots;
    MDS_HIP(hipMemcpyAsync(obs, (const char*)obs_log + (size_t)last * row, row, hipMemcpyDeviceToDevice, st));
  }
  return MDS_OK;
}

int mds_step_nominal(mds_handle* h, double t, void* obs, void* action, void* stream) {
  MDS_DEV(h);
  if (!h || !obs) return fail(MDS_EINVAL, "mds_step_nominal: null argument");
  if (h->cbf_nominal != 1 && h->cbf_nominal != 2)
    return fail(MDS_ESTATE, "mds_step_nominal: select the LQR-omega (1) or LQR-yank-omega (2) controller with mds_cbf_set_nominal first");
  if (h->cfg.dtype == MDS_F16) return fail(MDS_EUNSUPPORTED, "mds_step_nominal: fp16 storage");
  // no action wanted: the one-step instance of the whole-rollout kernel does LQR + low level + physics in one launch
  // (212 B per drone-step instead of 392 B over two launches: 34 / 48 us -> 18 us at C3)
  if (!action && h->has_traj && h->traj_mode == 1 && !h->envfx)
    return rollout_fused(h, t, 1, nullptr, obs, stream, h->cbf_nominal == 2 ? 3 : 2, "mds_step_nominal");
  return step_nominal_lowlevel(h, t, obs, nullptr, action, (hipStream_t)stream);
}


// ------------------------------------------------------------------------------------------------------------------------------
// FedCE system identification and the decentralised LQR (mds_fedce_kernels.hip)
// ------------------------------------------------------------------------------------------------------------------------------
int mds_fedce_supported(const mds_config* cfg) {
  if (!cfg) return fail(MDS_EINVAL, "mds_fedce_supported: null config");
  if (cfg->dtype == MDS_F16) return fail(MDS_EUNSUPPORTED, "FedCE / dLQR: fp16 storage is not built (f32 / f64 only)");
  if (cfg->dtype == MDS_F32C) return fail(MDS_EUNSUPPORTED, "FedCE / dLQR: the compensated MDS_F32C dtype is not built (f32 / f64 only)");
  if (cfg->integrator != MDS_INTEGRATOR_EULER) return fail(MDS_EUNSUPPORTED, "FedCE / dLQR: RK4 is not built (explicit Euler only)");
  if (cfg->physics != MDS_PHYSICS_DYN && cfg->physics != MDS_PHYSICS_DYN_DRAG)
    return fail(MDS_EUNSUPPORTED, "FedCE / dLQR: ground effect / downwash are not built (DYN / DYN_DRAG only)");
  if (cfg->num_drones < 1 || cfg->num_drones > kFedceMaxD) return fail(MDS_EUNSUPPORTED, "FedCE / dLQR: 1 <= num_drones <= 16 only");
  return MDS_OK;
}

static int fedce_ready(mds_handle* h, const char* who) {
  if (!h) return fail(MDS_EINVAL, who);
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  // both or none: fedce_P alone says "initialised" to the other entry points
  return h->mem.alloc_all({{&h->fedce_P, (size_t)h->n * 256 * sizeof(double)}, {&h->fedce_theta, (size_t)h->n * 12 * sizeof(double)}});
}

// theta [16,12] (row-major) -> the 12 free entries (project_theta)
static void fedce_project(const double* th, double f[12]) {
  f[0] = th[1 * 12 + 6];
  f[1] = th[0 * 12 + 7];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) f[2 + 3 * a + b] = th[(13 + b) * 12 + 3 + a];
  f[11] = th[12 * 12 + 8];
}
static void fedce_expand(const double f[12], double* th) {
  for (int k = 0; k < 192; ++k) th[k] = 0.0;
  for (int k = 0; k < 3; ++k) {
    th[(3 + k) * 12 + k] = 1.0;          // A[k, 3+k]
    th[(6 + k) * 12 + 9 + k] = 1.0;      // A[9+k, 6+k]
  }
  th[1 * 12 + 6] = f[0];
  th[0 * 12 + 7] = f[1];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) th[(13 + b) * 12 + 3 + a] = f[2 + 3 * a + b];
  th[12 * 12 + 8] = f[11];
}

int mds_fedce_init(mds_handle* h, const double P0[256], const double theta0[192]) {
  MDS_DEV(h);
  if (!h || !P0 || !theta0) return fail(MDS_EINVAL, "mds_fedce_init: null argument");
  if (int rc = fedce_ready(h, "mds_fedce_init")) return rc;
  double f[12];
  fedce_project(theta0, f);
  std::vector<double> P((size_t)h->n * 256), th((size_t)h->n * 12);
  for (size_t i = 0; i < (size_t)h->n; ++i) {
    memcpy(&P[i * 256], P0, 256 * sizeof(double));
    memcpy(&th[i * 12], f, 12 * sizeof(double));
  }
  MDS_HIP(hipMemcpy(h->fedce_P, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice));
  MDS_HIP(hipMemcpy(h->fedce_theta, th.data(), th.size() * sizeof(double), hipMemcpyHostToDevice));
  return MDS_OK;
}

int mds_fedce_get(mds_handle* h, double* theta_host, double* P_host) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_fedce_get: null handle");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->fedce_P) return fail(MDS_ESTATE, "mds_fedce_get: call mds_fedce_init first");
  MDS_HIP(hipDeviceSynchronize());
  if (P_host) MDS_HIP(hipMemcpy(P_host, h->fedce_P, (size_t)h->n * 256 * sizeof(double), hipMemcpyDeviceToHost));
  if (theta_host) {
    std::vector<double> f((size_t)h->n * 12);
    MDS_HIP(hipMemcpy(f.data(), h->fedce_theta, f.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)h->n; ++i) fedce_expand(&f[i * 12], theta_host + i * 192);
  }
  return MDS_OK;
}

int mds_fedce_set(mds_handle* h, const double* theta_host, const double* P_host) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_fedce_set: null handle");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->fedce_P) return fail(MDS_ESTATE, "mds_fedce_set: call mds_fedce_init first");
  MDS_HIP(hipDeviceSynchronize());
  if (P_host) MDS_HIP(hipMemcpy(h->fedce_P, P_host, (size_t)h->n * 256 * sizeof(double), hipMemcpyHostToDevice));
  if (theta_host) {
    std::vector<double> f((size_t)h->n * 12);
    for (size_t i = 0; i < (size_t)h->n; ++i) fedce_project(theta_host + i * 192, &f[i * 12]);
    MDS_HIP(hipMemcpy(h->fedce_theta, f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return MDS_OK;
}

int mds_fedce_identify(mds_handle* h, int n_steps, const double* u_dev, int u_mode, const double* xdes_dev, int update, void* obs_log_dev,
                       double* pred_err_log_dev, double* theta_log_dev, void* obs_dev, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_fedce_identify: null handle");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (n_steps < 0 || (n_steps > 0 && !u_dev) || (u_mode != 0 && u_mode != 1)) return fail(MDS_EINVAL, "mds_fedce_identify: n_steps / u_dev / u_mode");
  if (!h->fedce_P) return fail(MDS_ESTATE, "mds_fedce_identify: call mds_fedce_init first");
  if (!aligned16(obs_log_dev) || !aligned16(obs_dev) || !aligned16(theta_log_dev) || !aligned16(pred_err_log_dev) || !aligned16(u_dev) ||
      !aligned16(xdes_dev))
    return fail(MDS_EALIGN, "mds_fedce_identify: u / xdes / log / obs buffers");
  hipStream_t st = (hipStream_t)stream;
  if (n_steps > 0) {
    const FedceModel fm = {h->cfg.M * h->cfg.G, h->cfg.G, h->cfg.M, {h->cfg.J[0], h->cfg.J[1], h->cfg.J[2]}, 1.0 / h->cfg.ctrl_freq};
    const dim3 grid = grid_for(h->n * 16, kFedceBlock);
    with_dtype_no_half(h->cfg.dtype, [&](auto DT) {         // f32 / f64 (mds_fedce_supported)
      using T = typename decltype(DT)::T;
      with_flags([&](auto DRAG) {
        k_fedce_identify<T, T, DRAG()><<<grid, kFedceBlock, 0, st>>>(params<T>(h).c, h->p64.c, fm, h->n, h->ld, n_steps, (T*)h->state, (const T*)h->origin,
                                                                     (T*)rpm_track(h), u_dev, u_mode, xdes_dev, update, h->fedce_P, h->fedce_theta,
                                                                     (T*)obs_log_dev, pred_err_log_dev, theta_log_dev);
      }, has_drag(h));
    });
    MDS_HIP(hipGetLastError());
  }
  if (obs_dev) {
    if (obs_log_dev && n_steps > 0) {
      const size_t obs_bytes = (size_t)h->n * kObsDim * elem_size(h->cfg.dtype);
      MDS_HIP(hipMemcpyAsync(obs_dev, (char*)obs_log_dev + (size_t)(n_steps - 1) * obs_bytes, obs_bytes, hipMemcpyDeviceToDevice, st));
    } else {
      return mds_get_obs(h, obs_dev, stream);
    }
  }
  return MDS_OK;
}

int mds_set_dlqr_gain(mds_handle* h, const double* K_host) {
  MDS_DEV(h);
  if (!h || !K_host) return fail(MDS_EINVAL, "mds_set_dlqr_gain: null argument");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  const int E = h->cfg.num_envs, D = h->cfg.num_drones;
  const size_t per = (size_t)48 * D * D, total = per * E;
  const size_t es = h->cfg.dtype == MDS_F64 ? sizeof(double) : sizeof(float);
  if (int rc = h->mem.alloc(&h->dlqr_K, total * es)) return rc;
  std::vector<double> kd(h->cfg.dtype == MDS_F64 ? total : 0);
  std::vector<float> kf(h->cfg.dtype == MDS_F64 ? 0 : total);
  for (size_t e = 0; e < (size_t)E; ++e)
    for (int j = 0; j < D; ++j)
      for (int q = 0; q < 4; ++q)
        for (int col = 0; col < 12 * D; ++col) {
          const double v = K_host[e * per + (size_t)(4 * j + q) * (12 * D) + col];
          const size_t at = dlqr_kidx(e, D, j, q, col);
          if (kd.size()) kd[at] = v;
          else kf[at] = (float)v;
        }
  MDS_HIP(hipDeviceSynchronize());
  MDS_HIP(hipMemcpy(h->dlqr_K, kd.size() ? (const void*)kd.data() : (const void*)kf.data(), total * es, hipMemcpyHostToDevice));
  return MDS_OK;
}

int mds_dlqr_compute(mds_handle* h, const void* obs, const void* des, void* u, void* action, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !des || (!u && !action)) return fail(MDS_EINVAL, "mds_dlqr_compute: null argument");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->dlqr_K) return fail(MDS_ESTATE, "mds_dlqr_compute: call mds_set_dlqr_gain first");
  if (!aligned16(u) || !aligned16(action)) return fail(MDS_EALIGN, "mds_dlqr_compute: u_dev/action_dev");
  const int E = h->cfg.num_envs, D = h->cfg.num_drones, epb = kFedceBlock / D;
  const dim3 grid((unsigned)((E + epb - 1) / epb));
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {           // f32 / f64 (mds_fedce_supported)
    using T = typename decltype(DT)::T;
    k_dlqr_compute<T, T><<<grid, kFedceBlock, 0, (hipStream_t)stream>>>(params<T>(h).c, (const T*)h->dlqr_K, E, D, (const T*)obs, (const T*)des, (T*)u,
                                                                        (T*)action);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_rollout_dlqr_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs_last, void* stream) {
  MDS_DEV(h);
  if (!h || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_dlqr_fused: null handle / n_steps");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->has_traj) return fail(MDS_ESTATE, "mds_rollout_dlqr_fused: call mds_set_lemniscate / mds_set_trajectory_segments first");
  if (!h->dlqr_K) return fail(MDS_ESTATE, "mds_rollout_dlqr_fused: call mds_set_dlqr_gain first");
  if (!aligned16(obs_log) || !aligned16(obs_last)) return fail(MDS_EALIGN, "mds_rollout_dlqr_fused: obs buffers");
  if (n_steps == 0) return MDS_OK;
  const int E = h->cfg.num_envs, D = h->cfg.num_drones, epb = kFedceBlock / D;
  const dim3 grid((unsigned)((E + epb - 1) / epb));
  const double dt = 1.0 / h->cfg.ctrl_freq;
  hipStream_t st = (hipStream_t)stream;
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {           // f32 / f64 (mds_fedce_supported)
    using T = typename decltype(DT)::T;
    with_flags([&](auto DRAG) {
      k_dlqr_rollout<T, T, DRAG()><<<grid, kFedceBlock, 0, st>>>(params<T>(h).c, (const T*)h->dlqr_K, E, D, h->ld, t0, dt, n_steps, h->traj_mode,
                                                                 (T*)h->state, (const T*)h->origin, (const T*)h->lem, SegTable{h->segs, h->nseg_total},
                                                                 h->tinfo, (T*)rpm_track(h), (T*)obs_log, (T*)obs_last);
    }, has_drag(h));
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// FedCE and the decentralised LQR on the 9-state thrust / body-rate model (mds_fedce_omega_kernels.hip)
// ------------------------------------------------------------------------------------------------------------------------------
int mds_fedce_omega_supported(const mds_config* cfg) {
  if (!cfg) return fail(MDS_EINVAL, "mds_fedce_omega_supported: null config");
  return mds_fedce_supported(cfg);
}

// W = V^-1 [13,13] by Gauss-Jordan with partial pivoting (host, float64); false if V is singular
static bool fo_invert(const double* V, double* W) {
  constexpr int R = kOmegaR;
  double a[R][2 * R];
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < R; ++k) {
      a[r][k] = V[r * R + k];
      a[r][R + k] = r == k ? 1.0 : 0.0;
    }
  for (int p = 0; p < R; ++p) {
    int best = p;
    for (int r = p + 1; r < R; ++r)
      if (fabs(a[r][p]) > fabs(a[best][p])) best = r;
    if (!(fabs(a[best][p]) > 0.0)) return false;
    if (best != p)
      for (int k = 0; k < 2 * R; ++k) std::swap(a[p][k], a[best][k]);
    const double d = a[p][p];
    for (int k = 0; k < 2 * R; ++k) a[p][k] /= d;
    for (int r = 0; r < R; ++r) {
      if (r == p) continue;
      const double m = a[r][p];
      for (int k = 0; k < 2 * R; ++k) a[r][k] -= m * a[p][k];
    }
  }
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < R; ++k) W[r * R + k] = a[r][R + k];
  return true;
}

static int fo_ready(mds_handle* h) {
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  // all three or none: fo_V alone says "initialised" to the other entry points
  const size_t rr = (size_t)h->n * kOmegaR * kOmegaR * sizeof(double), rm = (size_t)h->n * kOmegaR * kOmegaM * sizeof(double);
  return h->mem.alloc_all({{&h->fo_V, rr}, {&h->fo_W, rr}, {&h->fo_theta, rm}});
}

int mds_fedce_omega_init(mds_handle* h, const double V0[169], const double theta0[117]) {
  MDS_DEV(h);
  if (!h || !V0 || !theta0) return fail(MDS_EINVAL, "mds_fedce_omega_init: null argument");
  if (int rc = fo_ready(h)) return rc;
  constexpr size_t RR = kOmegaR * kOmegaR, RM = kOmegaR * kOmegaM;
  double W0[RR];
  if (!fo_invert(V0, W0)) return fail(MDS_EINVAL, "mds_fedce_omega_init: V0 is singular");
  std::vector<double> V((size_t)h->n * RR), W((size_t)h->n * RR), th((size_t)h->n * RM);
  for (size_t i = 0; i < (size_t)h->n; ++i) {
    memcpy(&V[i * RR], V0, RR * sizeof(double));
    memcpy(&W[i * RR], W0, RR * sizeof(double));
    memcpy(&th[i * RM], theta0, RM * sizeof(double));
  }
  MDS_HIP(hipDeviceSynchronize());
  MDS_HIP(hipMemcpy(h->fo_V, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice));
  MDS_HIP(hipMemcpy(h->fo_W, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice));
  MDS_HIP(hipMemcpy(h->fo_theta, th.data(), th.size() * sizeof(double), hipMemcpyHostToDevice));
  return MDS_OK;
}

int mds_fedce_omega_get(mds_handle* h, double* theta_host, double* V_host) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_fedce_omega_get: null handle");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->fo_V) return fail(MDS_ESTATE, "mds_fedce_omega_get: call mds_fedce_omega_init first");
  MDS_HIP(hipDeviceSynchronize());
  if (V_host) MDS_HIP(hipMemcpy(V_host, h->fo_V, (size_t)h->n * kOmegaR * kOmegaR * sizeof(double), hipMemcpyDeviceToHost));
  if (theta_host) MDS_HIP(hipMemcpy(theta_host, h->fo_theta, (size_t)h->n * kOmegaR * kOmegaM * sizeof(double), hipMemcpyDeviceToHost));
  return MDS_OK;
}

int mds_fedce_omega_get_cov(mds_handle* h, double* W_host) {
  MDS_DEV(h);
  if (!h || !W_host) return fail(MDS_EINVAL, "mds_fedce_omega_get_cov: null argument");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->fo_V) return fail(MDS_ESTATE, "mds_fedce_omega_get_cov: call mds_fedce_omega_init first");
  MDS_HIP(hipDeviceSynchronize());
  MDS_HIP(hipMemcpy(W_host, h->fo_W, (size_t)h->n * kOmegaR * kOmegaR * sizeof(double), hipMemcpyDeviceToHost));
  return MDS_OK;
}

int mds_fedce_omega_set(mds_handle* h, const double* theta_host, const double* V_host) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_fedce_omega_set: null handle");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->fo_V) return fail(MDS_ESTATE, "mds_fedce_omega_set: call mds_fedce_omega_init first");
  constexpr size_t RR = kOmegaR * kOmegaR;
  std::vector<double> W;
  if (V_host) {
    W.resize((size_t)h->n * RR);
    for (size_t i = 0; i < (size_t)h->n; ++i)
      if (!fo_invert(V_host + i * RR, &W[i * RR])) return fail(MDS_EINVAL, "mds_fedce_omega_set: a V is singular");
  }
  MDS_HIP(hipDeviceSynchronize());
  if (V_host) {
    MDS_HIP(hipMemcpy(h->fo_V, V_host, W.size() * sizeof(double), hipMemcpyHostToDevice));
    MDS_HIP(hipMemcpy(h->fo_W, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (theta_host) MDS_HIP(hipMemcpy(h->fo_theta, theta_host, (size_t)h->n * kOmegaR * kOmegaM * sizeof(double), hipMemcpyHostToDevice));
  return MDS_OK;
}

int mds_fedce_omega_identify(mds_handle* h, int n_steps, const double* u_dev, const double* xdes_dev, int update, void* obs_log_dev,
                             double* theta_log_dev, int32_t* status_dev, void* obs_dev, void* stream) {
  MDS_DEV(h);
  if (!h) return fail(MDS_EINVAL, "mds_fedce_omega_identify: null handle");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (n_steps < 0 || (n_steps > 0 && !u_dev) || update < 0 || update > 4) return fail(MDS_EINVAL, "mds_fedce_omega_identify: n_steps / u_dev / update");
  if (!h->fo_V) return fail(MDS_ESTATE, "mds_fedce_omega_identify: call mds_fedce_omega_init first");
  if (!aligned16(obs_log_dev) || !aligned16(obs_dev) || !aligned16(theta_log_dev) || !aligned16(status_dev) || !aligned16(u_dev) ||
      !aligned16(xdes_dev))
    return fail(MDS_EALIGN, "mds_fedce_omega_identify: u / xdes / log / status / obs buffers");
  hipStream_t st = (hipStream_t)stream;
  if (n_steps > 0) {
    const dim3 grid = grid_for(h->n * 16, kFedceBlock);
    with_dtype_no_half(h->cfg.dtype, [&](auto DT) {         // f32 / f64 (mds_fedce_supported)
      using T = typename decltype(DT)::T;
      // update 3 / 4: 1 / 2 in the covariance form (theta_update), its own instantiation; 0, 1, 2 launch what they always launched
      with_flags([&](auto DRAG, auto COV) {
        k_fedce_omega_identify<T, T, DRAG(), COV()><<<grid, kFedceBlock, 0, st>>>(params<T>(h).c, h->cfg.M * h->cfg.G, 1.0 / h->cfg.ctrl_freq, h->n, h->ld,
                                                                                  n_steps, (T*)h->state, (const T*)h->origin, (T*)rpm_track(h), (T*)h->ll,
                                                                                  u_dev, xdes_dev, update > 2 ? update - 2 : update, h->fo_V, h->fo_W,
                                                                                  h->fo_theta, (T*)obs_log_dev, theta_log_dev, status_dev);
      }, has_drag(h), update > 2);
    });
    MDS_HIP(hipGetLastError());
  }
  if (obs_dev) {
    if (obs_log_dev && n_steps > 0) {
      const size_t obs_bytes = (size_t)h->n * kObsDim * elem_size(h->cfg.dtype);
      MDS_HIP(hipMemcpyAsync(obs_dev, (char*)obs_log_dev + (size_t)(n_steps - 1) * obs_bytes, obs_bytes, hipMemcpyDeviceToDevice, st));
    } else {
      return mds_get_obs(h, obs_dev, stream);
    }
  }
  return MDS_OK;
}

int mds_set_dlqr_omega_gain(mds_handle* h, const double* K_host) {
  MDS_DEV(h);
  if (!h || !K_host) return fail(MDS_EINVAL, "mds_set_dlqr_omega_gain: null argument");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  const int E = h->cfg.num_envs, D = h->cfg.num_drones;
  const size_t per = (size_t)4 * kOmegaM * D * D, total = per * E;
  const size_t es = h->cfg.dtype == MDS_F64 ? sizeof(double) : sizeof(float);
  if (int rc = h->mem.alloc(&h->dlqr_omega_K, total * es)) return rc;
  std::vector<double> kd(h->cfg.dtype == MDS_F64 ? total : 0);
  std::vector<float> kf(h->cfg.dtype == MDS_F64 ? 0 : total);
  for (size_t e = 0; e < (size_t)E; ++e)
    for (int j = 0; j < D; ++j)
      for (int q = 0; q < 4; ++q)
        for (int col = 0; col < kOmegaM * D; ++col) {
          const double v = K_host[e * per + (size_t)(4 * j + q) * (kOmegaM * D) + col];
          const size_t at = dlqr_kidx_m<kOmegaM>(e, D, j, q, col);
          if (kd.size()) kd[at] = v;
          else kf[at] = (float)v;
        }
  MDS_HIP(hipDeviceSynchronize());
  MDS_HIP(hipMemcpy(h->dlqr_omega_K, kd.size() ? (const void*)kd.data() : (const void*)kf.data(), total * es, hipMemcpyHostToDevice));
  return MDS_OK;
}

int mds_dlqr_omega_compute(mds_handle* h, const void* obs, const void* des, void* u, void* action, void* stream) {
  MDS_DEV(h);
  if (!h || !obs || !des || (!u && !action)) return fail(MDS_EINVAL, "mds_dlqr_omega_compute: null argument");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->dlqr_omega_K) return fail(MDS_ESTATE, "mds_dlqr_omega_compute: call mds_set_dlqr_omega_gain first");
  if (!aligned16(u) || !aligned16(action)) return fail(MDS_EALIGN, "mds_dlqr_omega_compute: u_dev/action_dev");
  const int E = h->cfg.num_envs, D = h->cfg.num_drones, epb = kFedceBlock / D;
  const dim3 grid((unsigned)((E + epb - 1) / epb));
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {           // f32 / f64 (mds_fedce_supported)
    using T = typename decltype(DT)::T;
    k_dlqr_omega_compute<T, T><<<grid, kFedceBlock, 0, (hipStream_t)stream>>>(params<T>(h).c, (const T*)h->dlqr_omega_K, E, D, h->ld,
                                                                              (T)(1.0 / h->cfg.ctrl_freq), (T*)h->ll, (const T*)obs, (const T*)des,
                                                                              (T*)u, (T*)action);
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

int mds_rollout_dlqr_omega_fused(mds_handle* h, double t0, int n_steps, void* obs_log, void* obs_last, void* stream) {
  MDS_DEV(h);
  if (!h || n_steps < 0) return fail(MDS_EINVAL, "mds_rollout_dlqr_omega_fused: null handle / n_steps");
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  if (!h->has_traj) return fail(MDS_ESTATE, "mds_rollout_dlqr_omega_fused: call mds_set_lemniscate / mds_set_trajectory_segments first");
  if (!h->dlqr_omega_K) return fail(MDS_ESTATE, "mds_rollout_dlqr_omega_fused: call mds_set_dlqr_omega_gain first");
  if (!aligned16(obs_log) || !aligned16(obs_last)) return fail(MDS_EALIGN, "mds_rollout_dlqr_omega_fused: obs buffers");
  if (n_steps == 0) return MDS_OK;
  const int E = h->cfg.num_envs, D = h->cfg.num_drones, epb = kFedceBlock / D;
  const dim3 grid((unsigned)((E + epb - 1) / epb));
  const double dt = 1.0 / h->cfg.ctrl_freq;
  hipStream_t st = (hipStream_t)stream;
  with_dtype_no_half(h->cfg.dtype, [&](auto DT) {           // f32 / f64 (mds_fedce_supported)
    using T = typename decltype(DT)::T;
    with_flags([&](auto DRAG) {
      k_dlqr_omega_rollout<T, T, DRAG()><<<grid, kFedceBlock, 0, st>>>(params<T>(h).c, (const T*)h->dlqr_omega_K, E, D, h->ld, t0, dt, n_steps,
                                                                       h->traj_mode, (T*)h->state, (const T*)h->origin, (const T*)h->lem,
                                                                       SegTable{h->segs, h->nseg_total}, h->tinfo, (T*)rpm_track(h), (T*)h->ll,
                                                                       (T*)obs_log, (T*)obs_last);
    }, has_drag(h));
  });
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}
// ------------------------------------------------------------------------------------------------------------------------------
// The dLQR gains on the device (mds_care_kernels.hip): one Riccati problem per (env, connected component of Q's block graph)
// ------------------------------------------------------------------------------------------------------------------------------
}  // extern "C"

template <int M>
static int care_solve_gain(mds_handle* h, const char* who, const double* Q, const double* R, int max_iter, double* K_dev, int32_t* status_dev,
                           int32_t* iters_dev, void* stream) {
  constexpr int slot = M == 12 ? 0 : 1;
  char msg[256];
  auto bad = [&](int code, const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return fail(code, msg);
  };
  if (!h || !Q || !R || !status_dev) return bad(MDS_EINVAL, "null argument");
  MDS_DEV(h);
  if (int rc = mds_fedce_supported(&h->cfg)) return rc;
  const double* theta = M == 12 ? h->fedce_theta : h->fo_theta;
  if (!theta) return bad(MDS_ESTATE, M == 12 ? "call mds_fedce_init first" : "call mds_fedce_omega_init first");
  if (!aligned16(K_dev) || !aligned16(status_dev) || !aligned16(iters_dev)) return bad(MDS_EALIGN, "K_dev / status_dev / iters_dev");
  if (max_iter <= 0) max_iter = kCareMaxIter;
  const int E = h->cfg.num_envs, D = h->cfg.num_drones, nq = M * D, nr = 4 * D;
  // R: block diagonal in 4 x 4 blocks, every block inverted on the host with the solver's own Gauss-Jordan routine
  std::vector<double> tab((size_t)D * 16);
  for (int i = 0; i < nr; ++i)
    for (int j = 0; j < nr; ++j)
      if (i / 4 != j / 4 && R[(size_t)i * nr + j] != 0.0) return bad(MDS_EUNSUPPORTED, "R is not block diagonal in 4 x 4 blocks per drone");
  for (int d = 0; d < D; ++d) {
    double a[4 * 9], mcol[4], lad;
    int piv[4];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) a[i * 9 + j] = R[(size_t)(4 * d + i) * nr + 4 * d + j];
    if (!care_gj_inverse<9>(CareSerial{}, a, 4, mcol, piv, &lad)) return bad(MDS_EINVAL, "a 4 x 4 block of R is singular");
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) tab[(size_t)d * 16 + i * 4 + j] = a[i * 9 + j];
  }
  // Q: symmetric; the connected components of its M x M block graph are the problems
  double qmax = 0.0;
  for (size_t k = 0; k < (size_t)nq * nq; ++k) qmax = fmax(qmax, fabs(Q[k]));
  for (int i = 0; i < nq; ++i)
    for (int j = 0; j < i; ++j)
      if (!(fabs(Q[(size_t)i * nq + j] - Q[(size_t)j * nq + i]) <= 1e-12 * qmax)) return bad(MDS_EINVAL, "Q is not symmetric");
  int comp[kFedceMaxD];
  for (int d = 0; d < D; ++d) comp[d] = d;
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < a; ++b) {
      bool linked = false;
      for (int i = 0; i < M && !linked; ++i)
        for (int j = 0; j < M && !linked; ++j) linked = Q[(size_t)(M * a + i) * nq + M * b + j] != 0.0;
      if (linked && comp[a] != comp[b]) {
        const int from = comp[a], to = comp[b];
        for (int d = 0; d < D; ++d)
          if (comp[d] == from) comp[d] = to;
      }
    }
  CareGroups singles = {}, pairs = {};
  for (int c = 0; c < D; ++c) {
    int members[kFedceMaxD], cnt = 0;
    for (int d = 0; d < D; ++d)
      if (comp[d] == c) members[cnt++] = d;
    if (cnt > 2 || (cnt == 2 && M != 12)) {
      int at = snprintf(msg, sizeof(msg), "%s: Q couples drones", who);
      for (int k = 0; k < cnt && at < (int)sizeof(msg) - 8; ++k) at += snprintf(msg + at, sizeof(msg) - at, " %d", members[k]);
      snprintf(msg + at, sizeof(msg) - at, M == 12 ? ": components of more than two drones are not built" : ": coupled drones are not built for the 9-state model");
      return fail(MDS_EUNSUPPORTED, msg);
    }
    if (cnt == 1) singles.drone[singles.count++][0] = members[0];
    if (cnt == 2) {
      pairs.drone[pairs.count][0] = members[0];
      pairs.drone[pairs.count++][1] = members[1];
    }
  }
  const size_t q1 = (size_t)D * 16, q2 = q1 + (size_t)singles.count * M * M;
  tab.resize(q2 + (size_t)pairs.count * 4 * M * M);
  for (int g = 0; g < singles.count; ++g)
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < M; ++j) tab[q1 + ((size_t)g * M + i) * M + j] = Q[(size_t)(M * singles.drone[g][0] + i) * nq + M * singles.drone[g][0] + j];
  for (int g = 0; g < pairs.count; ++g)
    for (int i = 0; i < 2 * M; ++i)
      for (int j = 0; j < 2 * M; ++j)
        tab[q2 + ((size_t)g * 2 * M + i) * 2 * M + j] = Q[(size_t)(M * pairs.drone[g][i / M] + i % M) * nq + M * pairs.drone[g][j / M] + j % M];
  // device side: the table (uploaded only when Q or R changed: a call with the same ones only enqueues), the staging K, the gain buffer
  // (allocated before anything is uploaded or enqueued: a call that cannot get its memory changes nothing)
  const size_t per = (size_t)nr * nq, total = per * E;
  const size_t es = h->cfg.dtype == MDS_F64 ? sizeof(double) : sizeof(float);
  void** gain = M == 12 ? &h->dlqr_K : &h->dlqr_omega_K;
  std::vector<DevMem::Want> bufs = {{&h->care_tab[slot], ((size_t)D * 16 + (size_t)D * M * M * 2) * sizeof(double)},      // the largest a table gets
                                    {gain, total * es, true}};                                                            // no gain yet: an env that fails keeps zeros
  if (!K_dev) bufs.push_back({&h->care_K64[slot], total * sizeof(double)});
  if (int rc = h->mem.alloc_all(bufs)) return rc;
  if (!K_dev) K_dev = h->care_K64[slot];
  if (h->care_tab_host[slot] != tab) {
    MDS_HIP(hipDeviceSynchronize());
    MDS_HIP(hipMemcpy(h->care_tab[slot], tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    h->care_tab_host[slot] = tab;
  }
  hipStream_t st = (hipStream_t)stream;
  MDS_HIP(hipMemsetAsync(K_dev, 0, total * sizeof(double), st));
  MDS_HIP(hipMemsetAsync(status_dev, 0, (size_t)E * sizeof(int32_t), st));
  if (iters_dev) MDS_HIP(hipMemsetAsync(iters_dev, 0, (size_t)E * sizeof(int32_t), st));
  const double* Rinv_tab = h->care_tab[slot];
  if (singles.count) {
    constexpr int W = 2 * M, WAVES = CareShape<W>::WAVES;
    const long np = (long)E * singles.count;
    k_care_solve<W><<<dim3((unsigned)((np + WAVES - 1) / WAVES)), 64 * WAVES, 0, st>>>(E, D, singles, theta, Rinv_tab, Rinv_tab + q1, max_iter, K_dev,
                                                                                        status_dev, iters_dev);
  }
  if constexpr (M == 12) {
    if (pairs.count) {
      const long np = (long)E * pairs.count;
      k_care_solve<48><<<dim3((unsigned)np), 64, 0, st>>>(E, D, pairs, theta, Rinv_tab, Rinv_tab + q2, max_iter, K_dev, status_dev, iters_dev);
    }
  }
  const dim3 grid((unsigned)((total + 255) / 256));
  if (h->cfg.dtype == MDS_F64) k_care_commit<double, M><<<grid, 256, 0, st>>>(E, D, K_dev, status_dev, (double*)*gain);
  else k_care_commit<float, M><<<grid, 256, 0, st>>>(E, D, K_dev, status_dev, (float*)*gain);
  MDS_HIP(hipGetLastError());
  return MDS_OK;
}

extern "C" {
int mds_dlqr_solve_gain(mds_handle* h, const double* Q_host, const double* R_host, int max_iter, double* K_dev, int32_t* status_dev,
                        int32_t* iters_dev, void* stream) {
  return care_solve_gain<12>(h, "mds_dlqr_solve_gain", Q_host, R_host, max_iter, K_dev, status_dev, iters_dev, stream);
}

int mds_dlqr_omega_solve_gain(mds_handle* h, const double* Q_host, const double* R_host, int max_iter, double* K_dev, int32_t* status_dev,
                              int32_t* iters_dev, void* stream) {
  return care_solve_gain<kOmegaM>(h, "mds_dlqr_omega_solve_gain", Q_host, R_host, max_iter, K_dev, status_dev, iters_dev, stream);
}
#endif  // MDS_PART & 2

}  // extern "C"
