// pe_mcts_search.hpp -- the search itself (a part of pe_mcts.hip): the tree's records, MCTS.search
// for one env over either kind of sim cells (search_env) and the two search kernels.
#pragma once
#include "pe_mcts_cells.hpp"
#include "pe_mcts_rng.hpp"

namespace {

struct MNode {          // MCTSNode, mcts_custom_trainer.py:20-33
  double value;         // sum of rollout rewards (:133)
  int32_t visits;
  uint32_t untried;     // bits 0-2: len(untried_actions); action j at bits 3+3j (list order, :32)
  uint16_t kid[5];      // children in dict insertion order (:31, :124)
  uint16_t parent;      // 0xFFFF at the root
  uint8_t nkid, action, pad[2];
};
static_assert(sizeof(MNode) == kNodeBytes, "32-B tree records");

constexpr uint32_t kAllUntried = 5u | (0u << 3) | (1u << 6) | (2u << 9) | (3u << 12) | (4u << 15);

__device__ __forceinline__ MNode load_node(const MNode* T, int i) {
  MNode nd;
  const uint4* src = reinterpret_cast<const uint4*>(T + i);
  uint4* dst = reinterpret_cast<uint4*>(&nd);
  dst[0] = src[0];
  dst[1] = src[1];
  return nd;
}

__device__ __forceinline__ void store_node(MNode* T, int i, const MNode& nd) {
  const uint4* src = reinterpret_cast<const uint4*>(&nd);
  uint4* dst = reinterpret_cast<uint4*>(T + i);
  dst[0] = src[0];
  dst[1] = src[1];
}

__device__ __forceinline__ MNode fresh_node(int parent, int action) {
  MNode nd;
  nd.value = 0.0;
  nd.visits = 0;
  nd.untried = kAllUntried;  // list(range(5)) (:32)
#pragma unroll
  for (int j = 0; j < 5; ++j) nd.kid[j] = 0;
  nd.parent = (uint16_t)parent;
  nd.nkid = 0;
  nd.action = (uint8_t)action;
  nd.pad[0] = nd.pad[1] = 0;
  return nd;
}

__device__ __forceinline__ int kid_at(const MNode& nd, int j) {
  int v = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) v |= k == j ? nd.kid[k] : 0;
  return v;
}

// The node indices on a simulation's path (16 bits each), root first: the first 8 in the words
// pth0, pth1 of search_env, plen counts them all (a longer path's backpropagation walks the parent
// links).  Macros over search_env's locals: as a struct with push / at the same code schedules
// differently.
#define PUSH_PATH(idx)                                                 \
  do {                                                                 \
    if (plen < 4) pth0 |= (uint64_t)(idx) << (16 * plen);              \
    else if (plen < 8) pth1 |= (uint64_t)(idx) << (16 * (plen - 4));   \
    ++plen;                                                            \
  } while (0)
#define PATH_AT(k) ((int)((((k) < 4 ? pth0 : pth1) >> (16 * ((k) & 3))) & 0xFFFFu))

// MCTS.search (:91-139) for env e with its sim cells in `cs`.  The four phases of a
// simulation are one loop of sim steps: each iteration picks the step's action by
// the lane's current phase (tree descent, expansion, rollout) and all lanes then
// run the same sim step together, whatever phase each is in.
enum : int { PH_SELECT = 0, PH_EXPAND = 1, PH_ROLLOUT = 2, PH_DONE = 3 };

#ifdef PE_MCTS_PROF  // diagnostics build: shader-clock cycles per phase, summed per lane
__device__ unsigned long long g_mcts_prof[1 << 20][4];
#define PE_MP_DECL uint64_t pa = 0, pb = 0, pc = 0
#define PE_MP_T(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define PE_MP_ACC(a_, b_, c_, d_) \
  do {                            \
    pa += b_ - a_;                \
    pb += c_ - b_;                \
    pc += d_ - c_;                \
  } while (0)
#define PE_MP_STORE(e_)                                                     \
  do {                                                                      \
    if ((e_) < (1 << 20)) {                                                 \
      g_mcts_prof[e_][0] = pa;                                              \
      g_mcts_prof[e_][1] = pb;                                              \
      g_mcts_prof[e_][2] = pc;                                              \
      g_mcts_prof[e_][3] = rng.topups;                                      \
    }                                                                       \
  } while (0)
#else
#define PE_MP_DECL
#define PE_MP_T(v)
#define PE_MP_ACC(a_, b_, c_, d_)
#define PE_MP_STORE(e_)
#endif

template <class CS>
__device__ void search_env(const MctsArgs& a, int64_t e, CS& cs, uint32_t* ring) {
#pragma clang fp contract(off)
  const Scal s0 = unpack(a.st.scal[e]);
  const int total = s0.total;
  MNode* T = a.nodes + e * (int64_t)(a.n_sims + 1);
  NpStream rng;
  rng.open(a.rng + e * (int64_t)kRngStride, ring);
  Nbr nb;
  Sim s;
  s.x = s0.x;
  s.y = s0.y;
  cs.load(s, nb);
  const bool root_expl = (nb.expl >> 4) & 1u;

  store_node(T, 0, fresh_node(0xFFFF, 0xFF));
  int nn = 1;
  PE_MP_DECL;
  for (int sim = 0; sim < a.n_sims; ++sim) {
    s.x = s0.x;
    s.y = s0.y;
    s.step = s0.step;
    s.expl = s0.expl;
    s.cur_expl = root_expl;
    s.bonus = false;  // a fresh PlantOSEnv: completion_bonus_given False (:221-243)
    int node = 0, depth = 0, phase = PH_SELECT;
    uint64_t pth0 = 0, pth1 = 0;
    int plen = 1;  // the root, index 0
    double tot = 0.0;
    MNode nd = load_node(T, 0);
    PE_MP_T(t0);
    // 1.-2. tree descent and expansion: a few steps, one shared sim step
    while (phase != PH_ROLLOUT) {
      rng.top_up_if_low();
      int act = -1;
      if (phase == PH_SELECT) {
        // 1. selection (:106-114): descend while fully expanded
        if ((nd.untried & 7u) == 0u && nd.nkid > 0 && depth < a.max_depth) {
          // a fully expanded node has all 5 children: their records load together
          const double lv = a.logt[nd.visits];
          MNode ch[5];
#pragma unroll
          for (int j = 0; j < 5; ++j) ch[j] = load_node(T, nd.kid[j]);
          int bj = 0;
          double bw = 0.0;
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            double wgt;
            if (ch[j].visits == 0) {
              wgt = INFINITY;
            } else {
              const double exploitation = ch[j].value / (double)ch[j].visits;       // :55
              const double exploration = a.c * sqrt(lv / (double)ch[j].visits);    // :56
              wgt = exploitation + exploration;                                     // :57
            }
            if (j == 0 || wgt > bw) {  // max(): the first maximal child (:60)
              bj = j;
              bw = wgt;
            }
          }
          int bidx = nd.kid[0];
          MNode bn = ch[0];
#pragma unroll
          for (int j = 1; j < 5; ++j)
            if (bj == j) {
              bidx = nd.kid[j];
              bn = ch[j];
            }
          node = bidx;
          nd = bn;
          PUSH_PATH(node);
          act = nd.action;
        } else {
          phase = PH_EXPAND;
        }
      }
      if (phase == PH_EXPAND) {
        // 2. expansion (:117-125); depth is not advanced
        if ((nd.untried & 7u) > 0u && depth < a.max_depth) {
          const int cnt = (int)(nd.untried & 7u);
          const int k = rng.randint(cnt);
          act = (int)((nd.untried >> (3 + 3 * k)) & 7u);
          const uint32_t below = nd.untried & ((1u << (3 + 3 * k)) - 1u) & ~7u;
          const uint32_t above = (nd.untried >> (3 + 3 * (k + 1))) << (3 + 3 * k);
          nd.untried = below | above | (uint32_t)(cnt - 1);
          const int ci = nn++;
#pragma unroll
          for (int j = 0; j < 5; ++j)
            if (j == nd.nkid) nd.kid[j] = (uint16_t)ci;
          nd.nkid += 1;
          store_node(T, node, nd);
          store_node(T, ci, fresh_node(node, act));
          node = ci;
          PUSH_PATH(node);
        } else {
          phase = PH_ROLLOUT;
        }
      }
      if (phase == PH_ROLLOUT) break;
      bool te, tr;
      cs.load(s, nb);
      sim_step(a.rl, cs, s, total, act, nb, te, tr);
      if (phase == PH_SELECT) {
        depth += 1;
        if (te || tr) phase = PH_EXPAND;
      } else {
        phase = PH_ROLLOUT;
      }
    }
    PE_MP_T(t1);
    // 3. rollout (:141-168), depth counts on from the descent
    for (int d = depth; d < a.max_depth; ++d) {
      rng.top_up_if_low();
      cs.load(s, nb);
      int act;
      if (rng.random_lt_07()) {                                   // np.random.random() < 0.7 (:180)
        // _exploration_heuristic (:187-219): first strictly least-visited valid move
        int best = -1;
        uint32_t minv = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (nb.code[q] != (uint32_t)OBST && (best < 0 || nb.vis[q] < minv)) {
            best = q;
            minv = nb.vis[q];
          }
        }
        act = best >= 0 ? best : rng.randint(5);
      } else {
        act = rng.randint(5);                                     // :183
      }
      bool te, tr;
      const double r = sim_step(a.rl, cs, s, total, act, nb, te, tr);
      tot += r;
      if (te || tr) {
        if (s.expl >= total) tot += 500.0;  // exploration_percentage >= 100 (:160-163)
        break;
      }
    }
    PE_MP_T(t2);
    // 4. backpropagation (:130-134): the path's records load together when it is
    // short (the usual case), else walk the parent links
    if (plen <= 8) {
      MNode pb[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < plen) pb[k] = load_node(T, PATH_AT(k));
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < plen) {
          pb[k].visits += 1;
          pb[k].value += tot;
          store_node(T, PATH_AT(k), pb[k]);
        }
    } else {
      for (int i = node; i != 0xFFFF;) {
        MNode b = load_node(T, i);
        b.visits += 1;
        b.value += tot;
        store_node(T, i, b);
        i = b.parent;
      }
    }
    cs.undo();  // the next simulation starts from a fresh copy (:104)
    PE_MP_T(t3);
    PE_MP_ACC(t0, t1, t2, t3);
  }
  PE_MP_STORE(e);
  // best_action (:62-69)
  const MNode root = load_node(T, 0);
  int act;
  if (root.nkid == 0) {
    act = rng.randint(5);
  } else {
    int best = -1;
    double bq = 0.0;
    for (int j = 0; j < root.nkid; ++j) {
      const MNode ch = load_node(T, kid_at(root, j));
      const double q = ch.value / (double)(ch.visits > 1 ? ch.visits : 1);
      if (best < 0 || q > bq) {
        best = ch.action;
        bq = q;
      }
    }
    act = best;
  }
  rng.close();
  a.actions[e] = act;
  if (a.rorder || a.rvisits || a.rvalue) {
    for (int j = 0; j < 5; ++j) {
      const bool has = j < root.nkid;
      MNode ch;
      if (has) ch = load_node(T, kid_at(root, j));
      if (a.rorder) a.rorder[e * 5 + j] = has ? ch.action : -1;
      if (a.rvisits) a.rvisits[e * 5 + j] = has ? ch.visits : 0;
      if (a.rvalue) a.rvalue[e * 5 + j] = has ? ch.value : 0.0;
    }
  }
}

// Any G: sim cells in global memory.
__global__ __launch_bounds__(64) void pe_mcts_search_kernel(MctsArgs a) {
  __shared__ uint32_t ring[64 * kRing];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  if (a.mask && !a.mask[e]) return;
  GCells cs;
  cs.cw = a.cellw + e * (int64_t)a.g.GG;
  cs.lg = a.ulog + e * (int64_t)(a.max_depth + 4);
  cs.nlog = 0;
  cs.G = a.g.G;
  search_env(a, e, cs, ring + threadIdx.x);
}

// G <= 64: the workgroup's 64 sim envs live in LDS (lane-private regions with an
// odd dword stride, so lanes at the same cell hit different banks): the rollout's
// neighbour reads and updates never leave the CU.
__global__ __launch_bounds__(64) void pe_mcts_search_lds_kernel(MctsArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int lane = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * 64;
  const int ggp = a.ggp, ldsw = a.ldsp / 4, nchunk = ggp / 16;
  // cooperative copy of the 64 clones (coalesced 16-B reads)
  const int64_t nenv = (int64_t)a.n - e0 < 64 ? (int64_t)a.n - e0 : 64;
  const uint4* src = reinterpret_cast<const uint4*>(a.cellb + e0 * ggp);
  uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
  for (int64_t i = lane; i < nenv * nchunk; i += 64) {
    const int el = (int)(i / nchunk), k = (int)(i - (int64_t)el * nchunk);
    const uint4 v = src[i];
    uint32_t* d = l32 + el * ldsw + 4 * k;
    if (4 * k + 0 < ldsw) d[0] = v.x;
    if (4 * k + 1 < ldsw) d[1] = v.y;
    if (4 * k + 2 < ldsw) d[2] = v.z;
    if (4 * k + 3 < ldsw) d[3] = v.w;
  }
  __syncthreads();
  const int64_t e = e0 + lane;
  if (e >= a.n) return;
  if (a.mask && !a.mask[e]) return;
  LCells cs;
  cs.cb = lds + lane * a.ldsp;
  cs.pristine = reinterpret_cast<const uint4*>(a.cellb + e * ggp);
  cs.cw = a.cellw + e * (int64_t)a.g.GG;
  cs.csim = a.csim + e * (int64_t)a.g.GG;
  cs.csg = a.csg + e * (int64_t)a.g.GG;
  cs.G = a.g.G;
  cs.nchunk = nchunk;
  cs.ldsw = ldsw;
  cs.stamp = 1;
  search_env(a, e, cs, reinterpret_cast<uint32_t*>(lds + 64 * a.ldsp) + lane);
}

}  // namespace
