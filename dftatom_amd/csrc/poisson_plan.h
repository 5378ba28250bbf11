// poisson_plan.h -- the multigrid's layout: the descriptor the kernels read (MgDesc), the constants it is built from, and the
// planner that fills it.  Host-only and pure: no HIP call, no environment -- poisson.hip passes in the knobs and the occupancy
// queries, tests/test_poisson_plan.py passes in numbers.
#pragma once

#include <cstddef>
#include <functional>

#if defined(__HIPCC__)
#define DFTA_MG_HD __host__ __device__
#else
#define DFTA_MG_HD
#endif

namespace dfta_mg {

constexpr int kMaxLevels = 24;
constexpr int kThreads = 256;
constexpr int kSeqBelow = 129;   // levels with n < 129 nodes: one lane, sequential, LDS-resident
constexpr int kWaveMaxN = 1025;  // staged levels up to this size are swept by the first wave alone (64 lanes: a quarter of the LDS traffic per warm-up step)
constexpr int kSeqCap = 144;     // LDS doubles per array for the sequential levels (65+33+17+9+5+3 = 132)
constexpr int kFuseMinLogC = 6;  // fuse the three sweeps of a visit of a global-memory level when every lane owns >= 64 nodes (knob POISSON_FUSE_MIN_LOGC)
constexpr int kStageMaxLogC = 5;   // chunked levels with <= 32 nodes per lane are swept from a copy in LDS (Phi, S)
constexpr int kStagePad = 128;     // one workgroup: doubles in front of each staged array (warm-up reads of the first lanes)
constexpr int kStageH = 24;        // group members: halo columns in front of every staged row (>= 96/C lanes, C >= 4)
constexpr int kStageRS = kThreads + kStageH;          // row stride of a member's staged part
constexpr int kStageArr = 8992;    // doubles per staged array: >= kStagePad + 8193 and >= kStageH + 32*kStageRS + 1
constexpr int kPad = 320;        // doubles of padding in front of every atom's level storage (warm-up reads of lane 0)
// the fused visit's warm-up (kWarm3 of an inclusion of poisson_kernels.inc): exact / tolerance mode
constexpr int kWarm3Exact = 112, kWarm3Tol = 32;

struct Lvl {
    int n;        // nodes
    int logC;     // chunk = 1 << logC
    int logT;     // lanes = 1 << logT   (n - 1 == C * T)
    int seq;      // 1: swept by a single lane in natural order
    int stage;    // swept from a copy in LDS (the CU's vector-memory path is the bound otherwise): 1 = one workgroup's level, 2 = shared level, 3 = one-wave level
    long off;     // offset of this level inside the per-atom level storage
    long soff;    // sequential levels: offset inside the LDS-resident copy
    double d;     // deltaGridLevel[l]
};

struct MgDesc {
    int levels;
    int G;           // workgroups per atom (power of two); 1: the whole solve runs in one workgroup
    int logG;
    int dbg;         // $DFTA_POISSON_DBG, measurements only (results are garbage): 1 = the coarse workgroup skips its sweeps, 2 = the members skip their passes, 4 = no restriction / prolongation on the shared levels
    int res_kres;    // > 0: resident group (k_poisson_solve_res): levels 0 .. res_kres-1 live in the members' LDS; the level layout is that of G = 1
    int res_logC0;   // log2(nodes per lane) of level 0 in a member's stretch (kResG members x kResNT lanes)
    int fuse_min_logc;   // global-memory levels of one workgroup: fused visits (gs_fused3) from this many nodes per lane on
    int fuse_coop;       // ... and on the levels the G workgroups of an atom share (0: $DFTA_DEBUG POISSON_NOFUSE_COOP)
    int fuse3;    // visits of three sweeps on staged levels of one workgroup run as ONE fused pass (gs_lds3); 0: $DFTA_POISSON_NOFUSE3
    int fuse3w;   // ... and those of the one-wave levels with 257 .. 1025 nodes of the coarse section (cs_visit3); 0: POISSON_NOFUSE3 / POISSON_NOFUSE3_WAVE
    int predict;  // exact mode: the fused visits of the one-wave levels (cs_visit3) start 32 nodes ahead from predicted values and are checked at the hand-over between the lanes; 0: POISSON_NOPREDICT, 2: POISSON_PREDICT_FUZZ (every prediction spoilt: every visit is repeated)
    unsigned long long* pred_ctr;   // device: [0] visits checked, [1] visits repeated (set by the solver after the plan is made)
    int nofold;   // DFTA_POISSON_NOFOLD: restriction / prolongation as separate passes even where they could be folded into a staged copy-in
    int fold_lds; // the folded restriction reads the finer level from the staging memory where its visit has just left it (POISSON_NOFOLD_LDS: from global)
    int kcoop;       // levels 0 .. kcoop-1 are swept by all G workgroups together (256 G lanes), the others by workgroup 0
    int spin_max;    // bound of the group barriers' spin loops (Atom::spin_max)
    long per_atom;   // doubles per atom and per array (sum of n)
    // Coarse section (coarse_section): levels cs_top .. levels-1 of a V-cycle are handled by the first wave of
    // workgroup 0 alone, entirely in LDS.  -1: off.  cs_phi / cs_src: offsets of a level's arrays inside the staging memory
    // (doubles), cs_lc: log2(nodes per lane) of its 64-lane interleaved layout, or -1 for natural order.
    int cs_top;
    int xw_top;      // exact mode: levels xw_top .. levels-1 (65, 33, 17, 9, 5, 3 nodes) of the coarse section with their nodes in registers (xw_section); -1: off
    int rc_src[6];   // ... offsets (doubles, inside the staging memory) of the sources of levels rc_top .. rc_top + 5 (256 C entries each)
    int adaptive;    // DFTA_POISSON_ADAPTIVE: stop the V-cycles at the round-off floor (run_cycles / res_cycles)
    int rc_top;      // tolerance mode, resident groups: the coarse workgroup runs levels rc_top .. levels-1 of a V-cycle with their nodes in registers (coarse_resident_cycle); -1: off
    int cs_phi[kMaxLevels], cs_src[kMaxLevels], cs_lc[kMaxLevels];
    Lvl lv[kMaxLevels];
};

constexpr int kXchg = 128;       // doubles per member and buffer of the boundary exchange (<= 96 halo nodes; the first node in the last one)
// per atom: [6 G + 2] partial sums of the members and the published state, [kGrpBuf G] slots of the fast sum, [kGrpBuf G kXchg] boundary
// nodes exchanged between neighbours in the middle of a staged visit
// fast-sum slots and boundary-exchange buffers rotate over kGrpBuf sets (round 3: 8, was 3): a member resets its part of the set half a
// rotation away, so that a reset has several exchanges to land before the slot is used again (see kResBuf below)
constexpr unsigned kGrpBuf = 8;
DFTA_MG_HD constexpr size_t group_part_doubles(int G) { return (size_t)(6 + kGrpBuf) * G + 2 + (size_t)kGrpBuf * G * kXchg; }

constexpr int kResNT = 128;                    // sweeping lanes of a member (its first two waves; all four move data)
constexpr int kResG = 32;                      // members per atom
constexpr int kResWG = kResG + 1;              // + the coarse workgroup (participant kResG of every exchange)
// the second configuration (poisson_kernels.inc under DFTA_MG_RES16 shadows the three above with these)
constexpr int kRes16NT = 256, kRes16G = 16, kRes16WG = kRes16G + 1;
constexpr int kResX = 272;                     // payload doubles per participant and buffer
constexpr int kResMaxShared = 4;
constexpr int kResXTail = 0, kResXSrc = 128, kResXHead = 256, kResXS0 = 266;
// Exchange buffers in rotation.  A slot holds a sentinel until its datum arrives; the owner resets its slots of buffer (s + kResBuf / 2)
// while exchange s completes -- a buffer nobody has touched for kResBuf / 2 exchanges and nobody will for as many.  (Three buffers, as
// in the staged groups above, leave one exchange between a reset and the slot's next use: an agent-scope store can overtake an
// earlier one on its way to another XCD, and a reader that still saw the datum of three exchanges ago took it for the new one --
// observed as rare run-to-run differences of the V-cycle count for He at 16385 nodes, where exchanges follow each other within 3 us.)
constexpr unsigned kResBuf = 16;
DFTA_MG_HD constexpr size_t res_slot_doubles() { return (size_t)kResBuf * kResWG * 4 + (size_t)kResBuf * kResWG * kResX; }

// $DFTA_DEBUG knobs of the multigrid, parsed once per creation (poisson.hip: read_knobs)
struct PoissonKnobs {
    bool group_set = false;      // POISSON_GROUP is present ...
    int group = -1;              // ... and, where its value is valid for the batch, log2 of the forced group size
    int res = -1, res16 = -1;    // POISSON_RES / POISSON_RES16: -1 unset, 0 off, 1 on
    bool nostage = false, nostage_wave = false, nostage_shared = false;
    bool nocoarse = false, noxw = false, norc = false;
    bool nofuse3 = false, nofuse3_wave = false, nohalf129 = false;
    bool nopredict = false, predict_fuzz = false;
    bool nofold = false, nofold_lds = false, nofuse_coop = false;
    int fuse_min_logc = kFuseMinLogC;   // POISSON_FUSE_MIN_LOGC, never below kFuseMinLogC
    int dbg = 0;                 // POISSON_DBG
    bool plain_launch = false;   // POISSON_PLAIN_LAUNCH, or a profiler is attached (ROCP_TOOL_LIBRARIES)
    int fault = 0;               // FAULT_POISSON_MEMBER
    int mode = 0;                // POISSON_MODE: what dfta_poisson_create (no mode argument) builds
};

enum PlanKernel { kKernelSolve, kKernelSolveRes, kKernelSolveRes16 };

struct PlanInputs {
    int N = 0, levels = 0;       // the grid: nodes of the finest level, multigrid levels
    double delta = 0;
    int uniform = 0;
    int batch = 1;
    int force_logG = -1;         // >= 0: that many doublings of the workgroups per atom (0: one workgroup per atom); -1: chosen from the batch size
    int mode = 0;                // DFTA_POISSON_EXACT / _TOLERANCE / _ADAPTIVE (0 / 1 / 2)
    int num_cu = 0;
    // workgroups of 256 threads of that kernel (of the mode's variant) a compute unit holds at once; < 0: the query failed
    std::function<int(PlanKernel)> occupancy;
    PoissonKnobs knobs;
};

struct PoissonPlan {
    MgDesc D = {};               // the kernels read a copy of it: every member defined
    bool resident = false;       // k_poisson_solve_res: the shared levels live in the members' LDS
    bool res16 = false;          // ... in its second configuration: 17 workgroups per atom
    bool plain_launch = false;   // groups started with an ordinary launch instead of a cooperative one (profilers, see plan_poisson)
    int fault = 0;               // FAULT_POISSON_MEMBER (tests): the last member of every group never arrives
    bool tol = false;            // tolerance mode: the kernels of namespace mg_tol (32-node warm-ups) instead of mg_exact
    bool adaptive = false;       // tolerance mode + the V-cycles stop at the round-off floor
    // elements of every allocation
    size_t n_level_store = 0;    // d_phi0, d_phi1, d_src: doubles each
    size_t n_cur = kMaxLevels;   // d_cur: ints
    size_t n_group_ctr = 0;      // unsigned
    size_t n_group_part = 0;     // doubles
    size_t n_res_slots = 0;      // doubles (resident)
    size_t n_res_spill = 0;      // doubles (res16)
    int occ_res = -1, occ_solve = -1;   // what the occupancy queries gave (-1: not asked)
    long seq_doubles = 0;        // LDS doubles per array of the sequential levels
    const char* error = nullptr; // set when the plan cannot be built
    int res_wg() const { return res16 ? kRes16WG : kResWG; }
};

// 0, or non-zero with plan->error set
int plan_poisson(const PlanInputs& in, PoissonPlan* plan);

}  // namespace dfta_mg
