// fvdb_internal.h — structures shared by the translation units of libfvdb_hip.so (not part of the C ABI).
#pragma once
#include "../../include/fvdb.h"

#include <hip/hip_runtime.h>

#include "common.h"  // PqGeom, which struct fvdb_pq below holds by value
#include "dev_owned.h"

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

struct fvdb_ctx {
  int device = 0;
  DevStream stream;  // declared before the buffers: it outlives them
  DevEvent ev0, ev1;
  int num_cus = 256;
  std::string err;   // last failure; written under err_mu (searches may fail on several host threads)
  std::mutex err_mu;
  void set_err(std::string m) {
    std::lock_guard<std::mutex> lk(err_mu);
    err = std::move(m);
  }
  HBuf h_stage;     // host->device staging for host-pointer entry points
  DBuf s_grid;      // fvdb_quality_grid_dev: the lists' prefix counts; grown and handed to the stream under grid_mu
  std::mutex grid_mu;
  int profiling = 0;
};

#define HIPCHK(ctx, call)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (ctx)->set_err(std::string(#call) + ": " + hipGetErrorString(e_));                      \
      return e_ == hipErrorOutOfMemory ? FVDB_E_OOM : FVDB_E_HIP;                             \
    }                                                                                         \
  } while (0)

#define FAIL(ctx, code, msg) \
  do {                       \
    (ctx)->set_err(msg);     \
    return (code);           \
  } while (0)

static inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

struct fvdb_store {
  fvdb_ctx* ctx = nullptr;
  uint32_t d = 0, dpad = 0;
  uint64_t rows = 0, cap = 0;
  uint32_t dtype = FVDB_F32;  // element of a stored row: FVDB_F32, or FVDB_F16 (rounded to nearest even at append)
  DBuf rows_buf;              // [cap][dpad] of it
  void* data = nullptr;       // rows_buf.p, as the kernels' argument lists take it
  bool f16() const { return dtype == FVDB_F16; }
  size_t row_bytes() const { return (size_t)dpad * (f16() ? 2 : 4); }
  DBuf s_q, s_cand, s_out, s_in;
};

struct fvdb_scorer {
  fvdb_store* store = nullptr;
  DevStream stream;  // private stream: scorers of different host threads run concurrently
  uint32_t max_B = 0, max_C = 0;
  DBuf q_buf;                  // d_q: [max_B][dpad]
  HBuf cand_buf, dist_buf;     // h_cand, h_dist: pinned, mapped
  float* d_q = nullptr;        // raw views of the three
  uint32_t* h_cand = nullptr;
  float* h_dist = nullptr;
  uint32_t* d_cand = nullptr;  // device aliases of the mapped buffers
  float* d_dist = nullptr;
  DBuf s_rows, s_in;  // private scratch: scorers are driven from different host threads
};

// the product quantizer (fvdb_pq.cpp), read by the indexes built over it (fvdb_ivfpq.cpp)
struct fvdb_pq {
  fvdb_ctx* ctx = nullptr;
  fvdb::PqGeom g{};        // g.ka = ksub_actual, 0 until trained
  uint32_t ksub = 0;
  uint32_t dmax = 0;       // pq_encode_kernel's instantiation: 8, 32 or 128
  uint32_t pad = 0;        // table rows in LDS carry one float of padding
  uint32_t lds_limit = 0;
  uint64_t version = 0;    // bumped whenever the codebooks change
  bool trained = false;
  DBuf books;              // [m][ksub][dims]: room for ksub * d floats
  DBuf s_rows, s_codes, s_refill;  // host-form scratch
  uint32_t ts() const { return g.ka + pad; }
  uint32_t m16() const { return (g.m + 15) / 16; }
  uint32_t qt() const {  // queries of a scan workgroup: the largest of 4, 2, 1 whose tables fit
    const uint64_t per = (uint64_t)g.m * ts() * 4;
    for (uint32_t q = 4; q; q >>= 1)
      if (per * q <= lds_limit) return q;
    return 0;
  }
};

// SQ8's refusal of rows and queries (fvdb_sq8.cpp): every element finite and every row's hi - lo finite in f32, else
// FVDB_E_NONFINITE
int sq8_check_rows(fvdb_ctx* ctx, const float* x, uint64_t n, uint32_t d);

// ---- allow-set masks (allow_masks.h) ---------------------------------------------------------
// A mask is a second liveness view of one index: pool words for an IVF index, per-node flags and the ascending list
// of allowed live nodes for a graph.  It is immutable once created and owns its buffers, so searches in any number of
// slots may read it at once.  `stamp` is the index's mutation counter at creation: a masked search compares it first.
struct fvdb_ivf;
struct fvdb_graph;
struct fvdb_mask {
  fvdb_ctx* ctx = nullptr;
  fvdb_ivf* ivf = nullptr;      // exactly one of ivf / graph is set
  fvdb_graph* graph = nullptr;
  uint64_t stamp = 0;
  uint64_t allowed_live = 0;    // rows (nodes) that are live in the index and in the allow-set
  uint32_t units = 0;           // pool blocks / graph nodes the buffers cover
  DBuf words;                   // IVF: valid[blk] & allow[blk], one word per pool block
  DBuf flags;                   // graph: deleted[node] | !allowed[node], one uint32_t per node
  DBuf nodes;                   // graph: allowed live node indices, ascending
};

// what allow_masks.h needs of a graph to build a mask and to scan under one, filled in by fvdb_graph.cpp
struct GraphMaskSource {
  fvdb_store* store;
  const uint32_t* deleted;  // [n]
  uint32_t n;
  uint64_t mutations;
};
int graph_mask_source(fvdb_graph* g, GraphMaskSource* out);
// the exact scan's inputs from the slot's scratch, enqueued on ctx's stream: the B queries at the store's row stride
// (q_dev itself when d == dpad, else a zero-padded copy) and room for part_bytes of partial lists
int graph_scan_inputs(fvdb_graph* g, fvdb_ctx* ctx, uint32_t slot, const float* q_dev, uint32_t B, size_t part_bytes,
                      const float** queries, uint64_t** part);
constexpr uint32_t kGraphSlots = 16;

// ---- the operand mirror of a graph's rows (flat_mfma_search.h) --------------------------------
// Owned by the graph, built and read by the filtered exact search.  Rows [0, built) of the store are mirrored; whatever
// renumbers or replaces rows (upload, vacuum) calls reset() and the next filtered search builds the mirror whole.
struct GraphFlatMirror {
  std::mutex mu;           // builds take turns; a search holds it only while it looks at / extends the mirror
  DBuf ops, xn, xmax;      // operand words [blocks][ksteps][64], |x|^2 [rows], the largest |x|^2 (one word)
  DBuf ctr[kGraphSlots];   // a slot's counters of its last search: pairs (8 bytes), fallbacks, unbounded
  uint64_t built = 0, cap_blocks = 0, builds = 0;
  uint32_t last_slot = 0;
  bool searched = false;
  float build_ms = 0.0f;   // the last build or extension, and the rows it covered
  uint64_t build_rows = 0;
  void reset() {
    std::lock_guard<std::mutex> lk(mu);
    built = 0;
  }
};
GraphFlatMirror* graph_flat_mirror(fvdb_graph* g);
