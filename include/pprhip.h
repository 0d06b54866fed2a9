/*
 * pprhip.h — C ABI of the MI355X-native Personalized-PageRank engine.
 *
 * This is the drop-in boundary for the hot path of
 * joezie/Personalized-PageRank-Algorithms-on-Neo4j (FORA single-source / top-k and
 * All-Pair-Backward-Search).  The reference has no FFI of its own; the seam is its three Java
 * interfaces plus the one-shot graph lift.  Every entry point below names the reference
 * interface it stands behind (paths relative to
 * /root/reference/src/main/java/joezie/fora_neo4j/).  INTEGRATION.md shows the JNI stub that
 * binds these symbols from the reference's Java classes.
 *
 * Conventions
 *   - plain C, opaque handles, caller-owned output buffers, no torch / STL types;
 *   - every function returns 0 (PPRHIP_OK) or a negative PPRHIP_ERR_* code; the message for the
 *     calling thread's last error is pprhip_last_error();
 *   - node ids are the dense mapped ids 0..n-1 (the harness assumes this too: Gen_Util.java:99-107);
 *   - all arithmetic on reserve / residue is IEEE double, as in the reference;
 *   - one handle belongs to one GPU and is used by one thread at a time (the reference objects
 *     are single-threaded and keep per-query state in fields, e.g. Forward_Push.java:33-43);
 *   - output pointers documented "may be NULL" leave the result resident in HBM; fetch it later
 *     with pprhip_get_reserve / pprhip_get_residue;
 *   - there is NO CPU fallback: every compute entry point fails with PPRHIP_ERR_NO_DEVICE when
 *     no gfx950 device is usable.
 *
 * Environment.  libpprhip.so reads these six variables and no others:
 *   PPRHIP_HOST_THREADS=<n>      host threads of the graph lift and the index finalisation (default: the CPU affinity /
 *                                cgroup quota of the process, at most 64)
 *   PPRHIP_BATCH_WORKSPACES=<n>  query workspaces of the batch driver, 16-48 (default 32; 0.33 GB each at R-MAT 22);
 *                                the batched weighted FORA calls: queries in flight, 1-16 (default 16)
 *   PPRHIP_BATCH_THREADS=0|1     batched top-k / All-Pair's third tier: one host thread per slot (default 1) or one in all
 *   PPRHIP_SHARD_CUT=count|work  target ranges of the sharded All-Pair: equal counts, or cut by measured work (default:
 *                                by work when equal counts would leave a rank more than 1.15 x the mean)
 *   PPRHIP_COMM_TIMEOUT_S=<s>    time limit of an exchange between ranks (default 1800)
 *   PPRHIP_RCCL_LIB=<path>       the librccl.so to load on first multi-GPU use (default: the loader's search)
 * (HIP_FORCE_DEV_KERNARG=1, a HIP runtime variable, is what the launchers set before the runtime starts: INTEGRATION.md.)
 * Fault injection, layout / driver variants, diagnostics on stderr and the measurement switches of the A/B runs exist only
 * in libpprhip_hooks.so - the same sources built with -DPPRHIP_TEST_HOOKS (make builds both) - which the tests that need
 * them and tools/exp load; the product ignores those variables.
 */
#ifndef PPRHIP_H
#define PPRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPRHIP_OK 0
#define PPRHIP_ERR_INVALID (-1)   /* bad argument (null pointer, id out of range, k < 1 ...) */
#define PPRHIP_ERR_NO_DEVICE (-2) /* no usable HIP device / device index out of range */
#define PPRHIP_ERR_HIP (-3)       /* a HIP runtime call failed; see pprhip_last_error() */
#define PPRHIP_ERR_OOM (-4)       /* host or device allocation failed */
#define PPRHIP_ERR_IO (-5)        /* file could not be read / parsed / written */
#define PPRHIP_ERR_STATE (-6)     /* call sequence error (e.g. topk round before reset) */

#define PPRHIP_VERSION 100

typedef struct pprhip_graph pprhip_graph_t;       /* device-resident CSR pair + per-query workspace */
typedef struct pprhip_edgelist pprhip_edgelist_t; /* host edge list produced by the ingest helpers */
typedef struct pprhip_index pprhip_index_t;       /* all-pair inverted index (host, CSR by source) */
typedef struct pprhip_results pprhip_results_t;   /* device-resident result vectors of a batched call (q x n doubles) */
typedef struct pprhip_comm pprhip_comm_t;         /* one rank of a multi-GPU group (RCCL communicator + its graph replica) */

/* Counters every compute call fills; all device-side counts, not estimates. */
typedef struct pprhip_stats {
  uint64_t pops;           /* frontier nodes pushed in sparse levels */
  uint64_t edge_pushes;    /* edges traversed in sparse levels */
  uint64_t enqueues;       /* nodes appended to a next frontier */
  uint64_t dead_end_pops;  /* pushed nodes with out-degree 0 (mass returned to the source) */
  uint64_t dense_nodes;    /* nodes pushed inside dense pull sweeps */
  uint32_t levels;         /* frontier levels run (sparse + dense) */
  uint32_t dense_levels;   /* levels run as dense pull sweeps */
  uint32_t rounds;         /* FORA: threshold rounds run (1 + halvings); top-k: delta rounds */
  uint32_t xl_targets;     /* All-Pair: searches that outgrew a workspace's lists and ran in the full-size pass */
  uint64_t mc_sources;     /* residue entries that started walks */
  uint64_t walks;          /* random walks run */
  uint64_t walk_steps;     /* edges followed by all walks (dead-end restarts included) */
  uint64_t select_passes;  /* radix-select passes over the reserve vector */
  double rsum;             /* sum of residues the walk budget was derived from */
  double rmax_final;       /* last push threshold used */
  double omega;            /* walk budget at rsum = 1 */
  double kth_value;        /* top-k: k-th largest estimate (0 when fewer than k entries) */
  double push_ms;          /* HIP-event time of the push phase */
  double mc_ms;            /* HIP-event time of the walk phase */
  double select_ms;        /* HIP-event time of the top-k selection */
  double total_ms;         /* HIP-event time of the whole call (device work only) */
  uint64_t push_bytes;     /* algorithmic bytes of the push phase (DESIGN.md byte model) */
  uint64_t mc_bytes;       /* algorithmic bytes of the walk phase */
  uint64_t select_bytes;   /* algorithmic bytes of the selection */
  double dominant_kernel_ms;    /* summed duration of the dominant kernel's launches */
  uint64_t dominant_kernel_bytes; /* algorithmic bytes those launches moved */
  uint32_t dominant_kernel_launches;
  uint32_t dominant_kernel_id;  /* PPRHIP_KERNEL_* */
  /* the same three figures for every kernel class, indexed by PPRHIP_KERNEL_* (HIP events on the
   * engine's stream around each launch; a sparse batch counts as one launch of class 2) */
  double class_ms[8];
  uint64_t class_bytes[8];
  uint32_t class_launches[8];
  uint64_t dense_edges;    /* out-edges of the nodes pushed inside dense pull sweeps: the edges a sweep had to serve,
                            * against dense_levels * m edges swept (useful-edge fraction of the sweeps) */
  uint64_t sweep_min_bytes; /* compulsory bytes of the dense sweeps: every byte a sweep has to read or write counted ONCE
                            * (index stream, each gathered contribution line once, row sums out and in, next
                            * contributions, the busy queries' residues) - a lower bound of the sweeps' memory traffic,
                            * whereas push_bytes' SURVEY 8(d) model counts one gather per edge and query */
  uint64_t walk_loads;      /* load instructions the walk kernel's waves issued (one 16-byte edge record per lane) ... */
  uint64_t walk_load_lanes; /* ... and the lanes those loads carried: 64 per load = every load a full wave */
} pprhip_stats_t;

#define PPRHIP_KERNEL_NONE 0
#define PPRHIP_KERNEL_DENSE_PULL 1
#define PPRHIP_KERNEL_SPARSE_PUSH 2
#define PPRHIP_KERNEL_WALK 3
#define PPRHIP_KERNEL_BACKWARD_BATCH 4
#define PPRHIP_KERNEL_DENSE_PULL_BATCH 5 /* one dense level for up to PPRHIP_BATCH queries */
#define PPRHIP_KERNEL_QUERY_SETUP 6      /* the short kernels around a query's phases: clearing its workspace, seeding a
                                          * round's frontier, residue sums, the walk plan, top-k selection (one "launch" =
                                          * one such group) */
#define PPRHIP_BATCH 16                  /* queries in flight in pprhip_fora_batch_single_source */

/* Engine tuning: the deterministic replacement of the reference's wall-clock push/walk balance
 * (Fora_Whole_Graph.java:35,75-79,93-103) and the sparse/dense switch.  Zero means "default". */
typedef struct pprhip_tuning {
  double c_walk_ns;        /* modelled cost of one random walk (reference constant: 400 ns) */
  double c_edge_ns;        /* modelled cost of one sparse edge push */
  double c_pop_ns;         /* modelled cost of one frontier pop */
  double c_level_ns;       /* modelled fixed cost of one level */
  double c_dense_edge_ns;  /* modelled cost per edge of a dense pull sweep */
  double c_dense_node_ns;  /* modelled cost per node of a dense pull sweep */
  double dense_frac;       /* a level runs dense when frontier_edges + frontier_nodes >= dense_frac * m */
  int32_t max_rounds;      /* cap on push rounds in auto mode (default 24) */
  int32_t max_halvings;    /* halvings of rmax one round may be followed by (default 6) */
  double halving_ratio;    /* a round is followed by 1 + k halvings when the modelled walk cost is still
                            * >= halving_ratio^k times the push cost so far (default 2) */
  int32_t prior_levels;    /* the first round starts below rmax0 by as many halvings as keep the a-priori walk
                            * bound c_walk * omega * (1 - alpha) * rmax * m >= prior_levels dense levels' cost
                            * (default 16; negative: always start at rmax0) */
  int32_t gs_blocks;       /* dense sweeps run block by block (Gauss-Seidel): rows are cut into gs_blocks blocks of equal
                            * in-edge count and a block reads the contributions the blocks before it have just written
                            * (default 2; 1: plain Jacobi sweeps) */
  double gs_frac;          /* ... while the frontier holds at least gs_frac * m edges + nodes (default 0.1, batch profile 0.05); thinner
                            * dense levels run as Jacobi sweeps */
} pprhip_tuning_t;

/* Parameters Algo_Conf derives (Algo_Conf.java:29-81). */
typedef struct pprhip_fora_conf {
  double alpha;      /* stop probability */
  double delta;      /* reserve threshold: 1/n (whole graph) or 1/k (top-k start) */
  double pfail;      /* failure probability: 1/n, or 1/n^2/ln(n div k) for top-k */
  double rsum;       /* initial residue sum: 1.0 */
  double min_delta;  /* top-k only: 1/n */
  int32_t k;         /* top-k only */
  uint32_t n;        /* node_amount */
  uint64_t m;        /* rel_amount */
} pprhip_fora_conf_t;

/* Parameter ranges.  Every entry point checks its numeric parameters before it looks at its handle and refuses a value
 * outside its range with PPRHIP_ERR_INVALID (pprhip_last_error names the function and the parameter); nothing reaches a
 * device.
 *   alpha (argument or conf->alpha)        finite, 0 < alpha < 1
 *   eps                                    finite, > 0
 *   rmax, min_rmax, the All-Pair threshold finite, >= 0 (0 is legal: a push at threshold 0 ends by underflow;
 *                                          pprhip_shard_target_cuts keeps its own threshold > 0)
 *   conf->delta                            finite, > 0
 *   conf->pfail                            whole-graph calls: finite, > 0; top-k calls: > 0 or the values
 *                                          pprhip_conf_fora_topk derives at n div k = 1 (+inf) and k > n (-0)
 *   conf->min_delta (top-k calls)          finite, > 0
 *   iters (pprhip_power_method)            >= 0 */

/* ---------------------------------------------------------------- errors / build info */
const char* pprhip_last_error(void);
int pprhip_version(void);
int pprhip_device_count(int* count_out);
/* Kernel-class times (pprhip_stats_t.class_ms, dominant_kernel_*) are measured with HIP events around every group of
 * launches; between the short kernels of the latency-bound paths those records cost 2-8 %, so they are an
 * option of the process: off unless PPRHIP_KERNEL_TIMER=1 is set or this is called with on != 0.  Off, the groups are
 * still counted (class_launches, class_bytes).  on == 2: only the dense sweeps are timed (PPRHIP_KERNEL_DENSE_PULL and
 * _DENSE_PULL_BATCH: two records per sweep of a millisecond), every other class counted - what bench.py's timed region
 * uses.  Not to be switched while a call is in flight.  Returns the old state (0, 1 or 2). */
int pprhip_set_kernel_timing(int on);
void pprhip_tuning_default(pprhip_tuning_t* t);
/* Cost-model constants for pprhip_fora_batch_single_source: a dense level costs a query 1/PPRHIP_BATCH
 * of a sweep, so the model values it lower and lets levels go dense earlier. */
void pprhip_tuning_batch(pprhip_tuning_t* t);
/* The batch profile for a call of q queries (Gen_Util.java:208-232 runs 50; sharded over 8 GPUs a call holds 6-7): with
 * fewer than PPRHIP_BATCH - 1 busy columns a dense level costs each query more, so the dense constants, dense_frac and
 * gs_frac grow with 14.5 / q, up to the single-query profile's values.  q >= 15: pprhip_tuning_batch.  The caller sets it
 * (pprhip_graph_set_tuning) before the call; every query of the call then is pprhip_fora_single_source under it. */
void pprhip_tuning_batch_for(int q, pprhip_tuning_t* t);

/* ---------------------------------------------------------------- parameter derivation (a10) */
/* Algo_Conf.set_conf_fora_whole_graph (Algo_Conf.java:45-53): delta = pfail = 1/n, rsum = 1. */
int pprhip_conf_fora_whole_graph(uint32_t n, uint64_t m, double alpha, pprhip_fora_conf_t* conf);
/* Algo_Conf.set_conf_fora_topk (Algo_Conf.java:71-81): min_delta = 1/n, delta = 1/k,
 * pfail = 1/n/n/ln(n div k) with integer division. */
int pprhip_conf_fora_topk(uint32_t n, uint64_t m, int k, double alpha, pprhip_fora_conf_t* conf);
/* Fora_Whole_Graph.java:86-87: rmax0 = eps*sqrt(delta/3/m/ln(2/pfail))/(1-alpha),
 * omega = (eps+2)*ln(2/pfail)/eps^2/delta. */
int pprhip_fora_whole_params(const pprhip_fora_conf_t* conf, double eps, double* rmax0, double* omega);
/* Fora_Topk.java:110-125,133 for one delta: eps' = eps/2; min_rmax, scaled rmax, omega. */
int pprhip_fora_topk_params(const pprhip_fora_conf_t* conf, double eps, double delta,
                            double* min_rmax, double* rmax_scaled, double* omega);

/* ---------------------------------------------------------------- graph ingest (host side) */
/* Seeded R-MAT edge list (Graph500 quadrants .57/.19/.19/.05), m = edge_factor << scale, labels
 * scrambled by a seeded permutation, parallel edges and self loops kept (the reference's
 * container is a multigraph: Forward_Push.java:119-139 visits every relationship). */
int pprhip_rmat_edges(int scale, int edge_factor, uint64_t seed, int32_t* src_out, int32_t* dst_out);
/* neo4j-admin-import CSVs (":ID,name" / ":START_ID,:END_ID,:TYPE"), id = node row index
 * (dataset/got/GOT_Nodes.csv, GOT_Rels.csv). */
int pprhip_edgelist_from_neo4j_csv(const char* nodes_csv, const char* rels_csv, pprhip_edgelist_t** out);
/* A Neo4j 3.x store directory read without a JVM: neostore.nodestore.db (15-byte records: in-use
 * bit, first relationship of the chain, dense flag) and neostore.relationshipstore.db (34-byte
 * records: first/second node, type, the four chain pointers); what PPR.createDb + setupAdjMatrix
 * get through the Neo4j kernel (PPR.java:52-60,136-152).  Node id = record id.  The adjacency
 * order is the relationship-chain order HeavyGraph sees.  Dense nodes (50 relationships or more: the node record
 * points to a chain of 25-byte relationship-group records, neostore.relationshipgroupstore.db, with separate
 * outgoing / incoming / loop chains per type) are read as well; a group of the wrong owner or a missing group store
 * is PPRHIP_ERR_IO. */
int pprhip_edgelist_from_neo4j_store(const char* store_dir, pprhip_edgelist_t** out);
int pprhip_edgelist_info(const pprhip_edgelist_t* e, uint32_t* n, uint64_t* m);
/* Out- (incoming = 0) or in-adjacency (incoming = 1) of an edge list in the order HeavyGraph
 * holds it: chain order for a store, newest relationship first for import CSVs. */
int pprhip_edgelist_build_csr(const pprhip_edgelist_t* e, int incoming, uint32_t* row_ptr_out /* n+1 */,
                              int32_t* col_idx_out /* m */);
int pprhip_edgelist_edges(const pprhip_edgelist_t* e, const int32_t** src, const int32_t** dst);
const char* pprhip_edgelist_node_name(const pprhip_edgelist_t* e, uint32_t id);
void pprhip_edgelist_destroy(pprhip_edgelist_t* e);
/* CSR by `key` (stable counting sort).  newest_first != 0 lists each row in descending edge
 * index, the order HeavyGraph inherits from Neo4j's relationship chains for got.db. */
int pprhip_csr_build(uint32_t n, uint64_t m, const int32_t* key, const int32_t* val, int newest_first,
                     uint32_t* row_ptr_out /* n+1 */, int32_t* col_idx_out /* m */);

/* ---------------------------------------------------------------- graph lift (a11) */
/* Replaces PPR.setupAdjMatrix + set_configuration (PPR.java:121-152): uploads the out- and
 * in-adjacency once.  in_* may be NULL, then the in-CSR is derived from the out-CSR. */
int pprhip_graph_create(uint32_t n, uint64_t m, const uint32_t* out_row_ptr, const int32_t* out_col_idx,
                        const uint32_t* in_row_ptr, const int32_t* in_col_idx, int device,
                        pprhip_graph_t** graph_out);
void pprhip_graph_destroy(pprhip_graph_t* g);
/* The host half of the lift alone, without a device: validation, the internal vertex order (nodes with in-edges first,
 * then out-degree descending, ties by id), both adjacencies in that order, the pull sweep's row-start flags and the
 * sliced copy of the in-adjacency - what pprhip_graph_create uploads.  It runs on `threads` host threads (0 = what the
 * process may use) and yields the same bytes with any count.  For inspection and tests; HeavyGraph's jagged arrays
 * (Diss. p.25) are the reference's counterpart of these arrays. */
typedef struct pprhip_lift pprhip_lift_t;
enum {
  PPRHIP_LIFT_NEW2OLD = 0,       /* int32[n] */
  PPRHIP_LIFT_OLD2NEW = 1,       /* int32[n] */
  PPRHIP_LIFT_OUT_ROW_PTR = 2,   /* uint32[n + 1] */
  PPRHIP_LIFT_OUT_COL_IDX = 3,   /* int32[m] */
  PPRHIP_LIFT_IN_ROW_PTR = 4,    /* uint32[n + 1] */
  PPRHIP_LIFT_IN_COL_IDX = 5,    /* int32[m] */
  PPRHIP_LIFT_NZ_ROWS = 6,       /* int32[]: nodes with in-edges */
  PPRHIP_LIFT_ZIN_ROWS = 7,      /* int32[]: nodes without in-edges that have out-edges */
  PPRHIP_LIFT_ROW_START_FLAGS = 8,   /* uint8[]: bit e = in-edge e is the first of its row */
  PPRHIP_LIFT_CHUNK_STARTS = 9,      /* uint32[]: rows that start before each 512-edge chunk */
  PPRHIP_LIFT_CROSS_BITS = 10,       /* uint64[]: bit j = row j holds the last edge of a chunk */
  PPRHIP_LIFT_SLICE_EDGE_BASE = 11,  /* uint64[S + 1] (empty: no sliced copy) */
  PPRHIP_LIFT_SLICE_SEG_BASE = 12,   /* uint64[S + 1] */
  PPRHIP_LIFT_SLICED_COL_IDX = 13,   /* int32[m], slice-major */
  PPRHIP_LIFT_SLICED_FLAGS = 14,     /* uint8[]: bit e = edge e of the sliced copy starts a segment */
  PPRHIP_LIFT_SLICED_CHUNK_STARTS = 15, /* uint32[] */
  PPRHIP_LIFT_SEG_ROW = 16,          /* uint32[segments]: row ordinal */
  PPRHIP_LIFT_SEG_OFF = 17,          /* uint32[segments]: first edge */
  /* the row-panel copy of the in-adjacency the single-query sweep walks (graphs from 2^26 edges on; they have no sliced
   * copy): panels of 8 192 consecutive rows with in-edges, a panel's in-edges sorted by (source, row); a panel of more
   * than 32 768 edges is cut into parts of equal edge counts; every part (item) padded to whole turns of 8 192 edges
   * with (0, 0xffff), a wave's 512 edges of a turn stored lane by lane (lane l: the edges l, l + 64, ...).  All empty
   * when the graph has none. */
  PPRHIP_LIFT_PANEL_SIZES = 18,      /* uint64[4]: panels, items, doubles of partial sums, edges with padding */
  PPRHIP_LIFT_PANEL_SRC = 19,        /* int32[edges]: sources */
  PPRHIP_LIFT_PANEL_ROW = 20,        /* uint16[edges]: row ordinal - first ordinal of the panel; 0xffff: padding */
  PPRHIP_LIFT_PANEL_ITEMS = 21,      /* uint32[items][4]: first edge / 8192, turns, panel, offset of the item's sums */
  PPRHIP_LIFT_PANEL_DESC = 22,       /* uint32[panels][4]: offset of the panel's sums, parts, rows, offset of their sums 32 at a time (or ~0) */
  PPRHIP_LIFT_PANEL_ITEM0 = 23       /* uint32[panels + 1]: first item of every panel */
};
int pprhip_graph_lift_host(uint32_t n, uint64_t m, const uint32_t* out_row_ptr, const int32_t* out_col_idx,
                           const uint32_t* in_row_ptr, const int32_t* in_col_idx, int threads,
                           pprhip_lift_t** lift_out);
/* *data_out points into the lift (valid until pprhip_lift_destroy) */
int pprhip_lift_array(const pprhip_lift_t* lift, int which, const void** data_out, uint64_t* bytes_out);
void pprhip_lift_destroy(pprhip_lift_t* lift);
/* A handle keeps the workspaces of every entry point it has served (allocating gigabytes per call would cost more than
 * the call): on first use of the batched entry points 16 query slots + interleaved arrays (R-MAT 22: 6.7 GB), on first
 * use of All-Pair the in-edge records, the dense per-workgroup vectors and the record buffer (R-MAT 22: 27 GB, R-MAT 24:
 * 80 GB).  pprhip_graph_release hands them back between phases of a job; the next call of that entry point allocates
 * them again.  The CSR pair, the walk records and the single-query workspace stay.  Not to be called while another
 * thread uses the handle. */
#define PPRHIP_RELEASE_ALL_PAIR 1u /* also the weighted All-Pair edge records (16 bytes per relationship) */
#define PPRHIP_RELEASE_BATCH 2u
#define PPRHIP_RELEASE_WALK_INDEX 4u /* the walk index (pprhip_walk_index_build): as pprhip_walk_index_drop */
#define PPRHIP_RELEASE_SWEEP 8u      /* the sweep cut's workspace (pprhip_sweep_cut: ranks, sort buffers, the profile) */
#define PPRHIP_RELEASE_SPARSE 16u    /* the sparse getters' workspace (tile counts, compacted entries, sort buffers) */
int pprhip_graph_release(pprhip_graph_t* g, unsigned what);
int pprhip_graph_info(const pprhip_graph_t* g, uint32_t* n, uint64_t* m, int* device);
/* HBM of the handle's device: bytes free and in all (hipMemGetInfo) - what a job holds at a point of its run is
 * total - free; bench.py reports it for the All-Pair samples (per rank in the sharded run). */
int pprhip_device_memory(const pprhip_graph_t* g, uint64_t* free_bytes, uint64_t* total_bytes);
int pprhip_graph_set_tuning(pprhip_graph_t* g, const pprhip_tuning_t* t);
int pprhip_graph_get_tuning(const pprhip_graph_t* g, pprhip_tuning_t* t);
/* Results of the last compute call that left them in HBM. */
int pprhip_get_reserve(pprhip_graph_t* g, double* reserve_out /* n */);
int pprhip_get_residue(pprhip_graph_t* g, double* residue_out /* n */);
/* ---- sparse results (beyond the reference)
 * The sparse form of a vector x (in original ids: what the dense getter returns) is its entries with x(v) > threshold,
 * each a pair (id, value) whose value has the bits the dense getter returns; compacted on the device, so that
 * 12 bytes per kept entry cross PCIe and not 8 per node.  threshold is finite and >= 0; threshold = 0 gives the
 * reference's HashMap<Long, Double> (entries > 0; -0.0 and NaN are never kept).  Orders:
 *   PPRHIP_SPARSE_BY_ID     id ascending: the ids are flatnonzero(x > threshold);
 *   PPRHIP_SPARSE_BY_VALUE  value descending, ties by id ascending - the order of the top-k calls.
 * The result is deterministic: the same bytes every run.  *count_out is the number of kept entries whatever cap is; the
 * first min(cap, count) entries of the ordered sequence are written (the convention of pprhip_walk_index_fetch and the
 * top-k calls), so by-value with a small cap is "the cap largest", and cap = 0 with null buffers is the counting
 * call.  ids_out and vals_out may each be NULL.  Checked before the handle is looked at, PPRHIP_ERR_INVALID: threshold
 * finite and >= 0, order in {0, 1}, a non-null count pointer (and offsets_out), no output buffer with cap == 0.  While a
 * query stream is open: PPRHIP_ERR_STATE.  The vector is not modified: the dense getters, pprhip_topk_select and
 * pprhip_sweep_cut give afterwards what they gave before.  The workspace (8 bytes per 1024 nodes and vector, 12 bytes per
 * kept entry, 24 more per entry for by-value) grows on demand and stays on the handle: pprhip_graph_release(
 * PPRHIP_RELEASE_SPARSE) and pprhip_graph_destroy free it. */
#define PPRHIP_SPARSE_BY_ID 0
#define PPRHIP_SPARSE_BY_VALUE 1
/* over the vector pprhip_get_reserve / pprhip_get_residue would return */
int pprhip_get_reserve_sparse(pprhip_graph_t* g, double threshold, int order, int32_t* ids_out, double* vals_out,
                              uint64_t cap, uint64_t* count_out);
int pprhip_get_residue_sparse(pprhip_graph_t* g, double threshold, int order, int32_t* ids_out, double* vals_out,
                              uint64_t cap, uint64_t* count_out);

/* ---------------------------------------------------------------- forward push (a1, a2) */
/* Forward_Push.computeWholeGraphPPR(Long s, Object rmax) (Forward_Push.java:63-142), run as a
 * frontier-synchronous schedule.  reserve_out / residue_out / rsum_out / stats may be NULL. */
int pprhip_forward_push(pprhip_graph_t* g, int32_t src, double alpha, double rmax, double* reserve_out,
                        double* residue_out, double* rsum_out, pprhip_stats_t* stats);
/* Forward_Push.forward_push_topk (Forward_Push.java:144-250): resumable two-threshold push.
 * reset = new Forward_Push(rsum = 1) + Q = {s}; each round resumes from the parked queue. */
int pprhip_fwdpush_topk_reset(pprhip_graph_t* g, int32_t src, double alpha);
int pprhip_fwdpush_topk_round(pprhip_graph_t* g, double min_rmax, double rmax, double* rsum_out,
                              pprhip_stats_t* stats);

/* ---------------------------------------------------------------- random walks (a3, a4) */
/* Monte_Carlo.random_walk / random_walk_no_zero_hop (Monte_Carlo.java:60-133) on the engine's
 * counter-based generator: walk (seed, stream, start, walk_idx) is a pure function, so the
 * terminal of every walk can be compared one by one. */
int pprhip_random_walk_batch(pprhip_graph_t* g, const int32_t* starts, const uint64_t* walk_idx, uint64_t count,
                             double alpha, uint64_t seed, uint32_t stream, int no_zero_hop,
                             int32_t* terminals_out, uint32_t* steps_out /* may be NULL */);

/* ---------------------------------------------------------------- FORA (a5, a6, a7) */
/* Fora_Whole_Graph.computeWholeGraphPPR(Long s, Object eps) (Fora_Whole_Graph.java:82-146).
 * n_rounds > 0 runs exactly that many threshold rounds (rmax0, rmax0/2, ...); 0 picks the thresholds
 * with the deterministic cost model of the tuning struct (the stand-in for the reference's wall-clock
 * loop, :93-103: first threshold, halvings per round, when to stop).  reserve_out may be NULL. */
int pprhip_fora_single_source(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf,
                              uint64_t seed, int n_rounds, double* reserve_out, pprhip_stats_t* stats);
/* Fora_Topk.computeTopKPPR + getTopKNodeIds (Fora_Topk.java:82-199).  Writes at most `cap`
 * (id, value) pairs ordered by value descending then id ascending; *n_out is the number the
 * reference's rule selects (all entries >= the k-th value, can exceed k on ties) and can exceed
 * cap.  reserve_out may be NULL.  After the call pprhip_get_reserve returns the estimate of the last round (what
 * reserve_out receives); the push state behind it (pprhip_get_residue, a following pprhip_fwdpush_topk_round) is
 * undefined: the engine may have pushed one threshold further than the last round the reference would run
 * (the next round's push runs ahead, beside the walks, and is dropped when the round is not needed). */
int pprhip_fora_topk(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                     int32_t* ids_out, double* vals_out, int cap, int* n_out, double* reserve_out,
                     pprhip_stats_t* stats);
/* Algo_Util.kth_ppr + retrieveTopK (Algo_Util.java:32-53, Fora_Topk.java:186-199) over the
 * reserve vector currently in HBM (entries == 0 do not exist in the reference's map). */
int pprhip_topk_select(pprhip_graph_t* g, int k, int32_t* ids_out, double* vals_out, int cap, int* n_out,
                       double* kth_out, pprhip_stats_t* stats);
/* Monte_Carlo.computeWholeGraphPPR (Monte_Carlo.java:136-158): omega = 3 ln(2/pfail)/eps^2/delta walks. */
int pprhip_monte_carlo(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                       double* ppr_out, pprhip_stats_t* stats);
/* q single-source FORA queries (the loop of Gen_Util.java:208-232 over Fora_Whole_Graph.
 * computeWholeGraphPPR), up to PPRHIP_BATCH of them in flight on this GPU.  Each query runs the
 * algorithm of pprhip_fora_single_source unchanged (same levels, thresholds, round count and, for
 * the same seed, the same walks: results agree up to the order of fp64 additions); dense levels of
 * concurrent queries share one sweep over the in-CSR, whose gathers fetch one 128-byte line per
 * vertex holding the contributions of all queries in flight.
 * reserve_out: q*n doubles (query-major) or NULL.  k > 0 additionally selects each query's top-k by
 * Algo_Util.kth_ppr's rule into ids_out/vals_out (q*k, rows padded with id -1 / value 0) and
 * n_out[i] (entries >= the k-th value; may exceed k on ties, NULL allowed).  per_query: q entries
 * or NULL; stats_sum: counters summed, kernel-class times of the whole call. */
int pprhip_fora_batch_single_source(pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                                    const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds,
                                    double* reserve_out, int k, int32_t* ids_out, double* vals_out, int* n_out,
                                    pprhip_stats_t* per_query, pprhip_stats_t* stats_sum);
/* Device-resident result store: the whole-graph vectors of up to `capacity` queries of a batched call stay in HBM
 * (capacity * n doubles; R-MAT 22, 128 queries: 4.3 GB of 288 GB), so that every query's getWholeGraphPPR()
 * (Whole_Graph_Util_Interface.java:8, read by Gen_Util.java:309) can still be served after its slot has been
 * reused, without moving q * n doubles over PCIe inside the call.  Slot i holds query i of the last call that
 * was given the store. */
int pprhip_results_create(pprhip_graph_t* g, int capacity, pprhip_results_t** results_out);
void pprhip_results_destroy(pprhip_results_t* r);
int pprhip_results_info(const pprhip_results_t* r, int* capacity, int* count, uint32_t* n);
/* vector of query i, caller's ids (n doubles) */
int pprhip_results_fetch(pprhip_results_t* r, int i, double* reserve_out);
/* vector of query i in sparse form ("sparse results" above) */
int pprhip_results_fetch_sparse(pprhip_results_t* r, int i, double threshold, int order, int32_t* ids_out,
                                double* vals_out, uint64_t cap, uint64_t* count_out);
/* every vector the store holds, as one CSR: offsets_out[count + 1] (always filled), row i = entries
 * [offsets[i], offsets[i + 1]) of vector i in the chosen order; *total_out = offsets[count]; the first min(cap, total)
 * entries of the concatenated rows are written.  An empty store gives offsets {0} and total 0. */
int pprhip_results_fetch_sparse_all(pprhip_results_t* r, double threshold, int order, uint64_t* offsets_out,
                                    int32_t* ids_out, double* vals_out, uint64_t cap, uint64_t* total_out);
/* sum of the vector of query i, computed on the device (a cheap mass check: 1 up to rounding when walks ran) */
int pprhip_results_sum(pprhip_results_t* r, int i, double* sum_out);
/* pprhip_fora_batch_single_source with the vectors kept in `keep` (q <= capacity); reserve_out may still be given. */
int pprhip_fora_batch_single_source_resident(pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                                             const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds,
                                             pprhip_results_t* keep, double* reserve_out, int k, int32_t* ids_out,
                                             double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                             pprhip_stats_t* stats_sum);

/* The batched driver behind a submit / wait pair (an extension: the reference's harness is synchronous,
 * Gen_Util.java:208-232).  A synchronous call ends with a drain - its last queries finish at different times and a
 * sweep costs the same for 2 busy columns as for 16 - so calls of PPR.java:179's 50 queries reach 0.90 of the rate of
 * long calls.  A stream keeps a driver thread on the handle: the slots a submission's last queries leave take the next
 * submission's first ones.  Every query runs as pprhip_fora_batch_single_source would run it (same seed and tuning,
 * same result); per submission: top-k blocks (k > 0: ids_out / vals_out [q * k], n_out [q] or NULL), and / or the
 * vectors in a device-resident store (`keep` slots keep_first .. keep_first + q - 1).  While a stream is open every
 * other entry point on the handle returns PPRHIP_ERR_STATE (one handle, one thread: here the driver's); outputs of a
 * submission may be read after its wait, a store after the close.  submit / wait may be called from any one thread. */
typedef struct pprhip_stream pprhip_stream_t;
int pprhip_fora_stream_open(pprhip_graph_t* g, double eps, const pprhip_fora_conf_t* conf, int k,
                            pprhip_stream_t** stream_out);
int pprhip_fora_stream_submit(pprhip_stream_t* s, const int32_t* srcs, int q, uint64_t seed, pprhip_results_t* keep,
                              int keep_first, int32_t* ids_out, double* vals_out, int* n_out, uint64_t* ticket_out);
/* blocks until every query of the submission has finished; stats_sum: its counters (total_ms = submit to finish).
 * A ticket can be waited for once; submissions nobody waits for are finished and released by the close. */
int pprhip_fora_stream_wait(pprhip_stream_t* s, uint64_t ticket, pprhip_stats_t* stats_sum);
/* finishes everything submitted, ends the driver thread and frees the stream.  (pprhip_graph_destroy on a graph whose
 * stream is still open ends the driver itself; the stream object then only remains to be freed by this call.) */
int pprhip_fora_stream_close(pprhip_stream_t* s);
/* FORA top-k (pprhip_fora_topk) for q sources, up to PPRHIP_BATCH of them in flight: every query runs
 * Fora_Topk's loop on delta unchanged (query i with seed + i), the dense levels of its forward_push_topk
 * rounds share sweeps with the other queries in flight.  ids_out/vals_out are q*k, rows padded with
 * id -1 / value 0 (entries beyond k that tie with the k-th value are dropped). */
int pprhip_fora_batch_topk(pprhip_graph_t* g, const int32_t* srcs, int q, int k, double eps, double alpha,
                           uint64_t seed, int32_t* ids_out, double* vals_out, pprhip_stats_t* stats_sum);

/* ---------------------------------------------------------------- seed sets (beyond the reference)
 * PPR personalized to a weighted node set, as Neo4j's PageRank takes it (sourceNodes; the reference passes one node,
 * Neo4j_Method.java:73-77).  seeds: n_seeds >= 1 original ids; weights: n_seeds finite values >= 0, or NULL (uniform).
 * Duplicates are summed, the weights normalized by their sum into p; zero weights are dropped.  An empty set, an id out
 * of range, a negative / NaN / infinite weight or weights summing to 0 is PPRHIP_ERR_INVALID, the graph untouched.
 * The target is pi_p of the walk that starts at a node drawn from p, stops with probability alpha per step and jumps
 * to a node drawn from p at a dead end: the push starts from r = p and lands every level's dead-end mass x on p
 * (r(s_i) += x p_i, with the threshold test of a push); a dead-end seed's share is resolved in closed form
 * (DESIGN.md §2 "Seed sets").  The walks of FORA are the single-source path's: they start at residue nodes with the
 * same counters and restart at their start node at a dead end (Monte_Carlo.java:87-90; the same walk quirk as the
 * single-source path).  A set of one seed reduces to the single-source call (same levels, rounds and walks, reserve
 * up to fp64 addition order).  One query at a time per handle (many per call: the batched calls below);
 * pprhip_get_reserve / _get_residue / pprhip_topk_select work on the result as after the single-source calls.
 * Generalized calls: pprhip_forward_push, pprhip_fora_single_source, pprhip_fora_topk. */
/* pprhip_forward_push from p; outputs as there. */
int pprhip_forward_push_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                              double alpha, double rmax, double* reserve_out, double* residue_out,
                              double* rsum_out, pprhip_stats_t* stats);
/* pprhip_fora_single_source from p (conf, eps, n_rounds, seed and the cost model as there); outputs as there. */
int pprhip_fora_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double eps,
                      const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds, double* reserve_out,
                      pprhip_stats_t* stats);
/* pprhip_fora_topk from p: the live seeds start parked, as {s} does for one source (Fora_Topk.java:117-118); outputs,
 * selection rule and the state pprhip_get_reserve / pprhip_topk_select see afterwards as there.  The push session
 * ends with the call (pprhip_fwdpush_topk_round needs a pprhip_fwdpush_topk_reset after it). */
int pprhip_fora_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                           double eps, const pprhip_fora_conf_t* conf, uint64_t seed, int32_t* ids_out,
                           double* vals_out, int cap, int* n_out, double* reserve_out, pprhip_stats_t* stats);
/* Batched seed sets: q sets in one call, kBatch (16) of them in flight on the handle's batch workspaces, their dense
 * levels sharing the batched sweeps as the single-source batched calls' do.  The sets are described like a CSR:
 * offsets holds q + 1 entries, offsets[0] == 0, non-decreasing; set i is seeds[offsets[i] .. offsets[i + 1]) with the
 * same slice of weights (weights NULL: every set uniform).  Every set is checked by the rules above before any device
 * work - the message names the set (", set i: ") - and so are the offsets; a failed check or q < 0 is
 * PPRHIP_ERR_INVALID with the handle untouched; q == 0 is an empty call.  While a query stream is open on the handle:
 * PPRHIP_ERR_STATE, as for every call. */
/* Query i is pprhip_fora_seeds(set i, eps, conf, seed, n_rounds): the same rounds, levels, dense levels and walks, the
 * vector equal up to fp64 addition order.  keep / reserve_out / k / ids_out / vals_out / n_out / per_query /
 * stats_sum as in pprhip_fora_batch_single_source_resident. */
int pprhip_fora_batch_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, const uint64_t* offsets,
                            int q, double eps, const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds,
                            pprhip_results_t* keep, double* reserve_out, int k, int32_t* ids_out, double* vals_out,
                            int* n_out, pprhip_stats_t* per_query, pprhip_stats_t* stats_sum);
/* Query i is pprhip_fora_topk_seeds(set i, eps, conf, seed + i) under the conf pprhip_fora_batch_topk builds
 * (pprhip_conf_fora_topk(n, m, k, alpha)); ids_out / vals_out (q*k) and stats_sum as in pprhip_fora_batch_topk. */
int pprhip_fora_batch_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights,
                                 const uint64_t* offsets, int q, int k, double eps, double alpha, uint64_t seed,
                                 int32_t* ids_out, double* vals_out, pprhip_stats_t* stats_sum);

/* ---------------------------------------------------------------- backward search (a8, a9) */
/* Backward_Search.backward_search_whole_graph(Long t) (Backward_Search.java:38-100). */
int pprhip_backward_push(pprhip_graph_t* g, int32_t target, double alpha, double rmax, double* reserve_out,
                         double* residue_out, pprhip_stats_t* stats);
/* Base_Whole_Graph.preprocessing(threshold, k) (Base_Whole_Graph.java:58-164) for the targets
 * [t_begin, t_end): backward search per target, entries >= threshold inverted into per-source
 * lists; k >= 0 keeps entries >= the k-th largest and sorts them descending, k < 0 keeps all in
 * target order.  The result covers all n sources for this shard of targets. */
int pprhip_all_pair_backward(pprhip_graph_t* g, double alpha, double threshold, int k, uint32_t t_begin,
                             uint32_t t_end, pprhip_index_t** index_out, pprhip_stats_t* stats);
/* Merge the shards of several target ranges (one per GPU) into one index, re-applying the k rule. */
int pprhip_index_merge(const pprhip_index_t* const* shards, int n_shards, int k, pprhip_index_t** merged_out);
/* Rebuild a shard from its arrays (what a rank receives from another rank before merging). */
int pprhip_index_from_arrays(uint32_t n, const uint64_t* offsets /* n+1 */, const int32_t* targets,
                             const double* values, pprhip_index_t** index_out);
int pprhip_index_info(const pprhip_index_t* ix, uint32_t* n, uint64_t* entries);
int pprhip_index_arrays(const pprhip_index_t* ix, const uint64_t** offsets /* n+1 */, const int32_t** targets,
                        const double** values);
/* Per-source text files "<t>\t<Double.toString(pi)>\n" (Base_Whole_Graph.java:118-126,152-156). */
int pprhip_index_write_dir(const pprhip_index_t* ix, const char* dir);
/* java.lang.Double.toString(d) as the reference's writers print it (shortest round-trip digits,
 * "1.0E-4" style outside [1e-3, 1e7)); returns the length written (without the NUL) or < 0. */
int pprhip_format_double(double d, char* buf, size_t cap);
void pprhip_index_destroy(pprhip_index_t* ix);

/* ---------------------------------------------------------------- multi-GPU
 * Queries (Gen_Util.java:208-232) and targets (Base_Whole_Graph.java:76-92) are independent: every GPU holds a
 * replica of the CSR (one pprhip_graph_t per GPU) and runs its share with the single-GPU code; nothing is exchanged
 * inside a query or a search.  Two exchanges close a call, both over RCCL (librccl is loaded on first use):
 * batched FORA gathers the per-query top-k blocks on rank 0; All-Pair, whose result is keyed by source
 * (Base_Whole_Graph.java:84-86), sends every entry (v, t, pi) to the rank that owns source v - partitioned on the
 * device, one message per peer (one xGMI link each), copied to the host once, by the owner that finalises it. */

/* One process, n_gpu GPUs, one host thread per GPU inside the call: query i runs on per_gpu[i mod n_gpu] exactly as
 * pprhip_fora_batch_single_source would run it (same seed, same walks), the top-k blocks are gathered on GPU 0.
 * ids_out / vals_out: q * k (rows padded with id -1 / value 0), n_out[q] or NULL, stats_per_gpu[n_gpu] or NULL.
 * Handles that share a device (a test set-up) exchange through in-process copies instead of RCCL. */
int pprhip_fora_batch(pprhip_graph_t* const* per_gpu, int n_gpu, const int32_t* srcs, int q, int k, double eps,
                      const pprhip_fora_conf_t* conf, uint64_t seed, int n_rounds, int32_t* ids_out, double* vals_out,
                      int* n_out, pprhip_stats_t* stats_per_gpu);
/* Base_Whole_Graph.preprocessing(threshold, k) over all n targets on n_gpu GPUs: GPU r searches the targets of
 * pprhip_shard_target_range(r) and owns the sources of the same range; returns the whole index (identical to
 * pprhip_all_pair_backward over [0, n) on one GPU). */
int pprhip_all_pair_backward_multi(pprhip_graph_t* const* per_gpu, int n_gpu, double alpha, double threshold, int k,
                                   pprhip_index_t** index_out, pprhip_stats_t* stats_per_gpu);

/* One process per GPU (torch.distributed, MPI, one JVM per GPU): rank 0 draws an id, hands its PPRHIP_COMM_ID_BYTES
 * bytes to every rank by any means, every rank creates its communicator (collective, like ncclCommInitRank). */
#define PPRHIP_COMM_ID_BYTES 128
int pprhip_comm_unique_id(void* id_out /* PPRHIP_COMM_ID_BYTES */);
int pprhip_comm_create(pprhip_graph_t* g, const void* id, int rank, int world, pprhip_comm_t** comm_out);
void pprhip_comm_destroy(pprhip_comm_t* c);
int pprhip_comm_info(const pprhip_comm_t* c, int* rank, int* world);
/* contiguous share [begin, end) of rank `rank` when [0, n) is cut into `world` ranges (targets and owned sources) */
int pprhip_shard_target_range(int rank, int world, uint32_t n, uint32_t* begin, uint32_t* end);
/* The target ranges a sharded All-Pair run searches: cuts_out[world + 1], rank r takes the targets
 * [cuts_out[r], cuts_out[r + 1]).  mode 0: equal counts (pprhip_shard_target_range); mode 1: by work - a pilot measures
 * the searches of the 16 targets with the most in-edges and of 48 more across the in-degree ranks on this handle,
 * every other target is estimated from its in-degree, and the cuts fall at equal shares of the running sum (a store
 * whose ids follow its in-degrees gives rank 0 every hub under equal counts: Base_Whole_Graph.java:76-92 iterates the
 * targets in id order); mode 2: what pprhip_all_pair_backward_sharded does - by work when equal counts would leave one
 * rank with more than 1.15 x the mean of the modelled work (skew_out, may be NULL), else equal counts.  The sources a
 * rank owns stay equal counts in every mode. */
int pprhip_shard_target_cuts(pprhip_graph_t* g, int world, double alpha, double threshold, int mode, uint32_t* cuts_out,
                             double* skew_out);
/* Collective: this rank searches its target range, entries are exchanged by owner of the source on the device, and
 * own_out receives the finished rows (k rule applied) of the sources this rank owns (rows of other sources empty).
 * stats: this rank's search; stats->mc_sources = entries it found, stats->select_bytes = bytes it received. */
int pprhip_all_pair_backward_sharded(pprhip_comm_t* c, double alpha, double threshold, int k, pprhip_index_t** own_out,
                                     pprhip_stats_t* stats);
/* Collective: every rank contributes `rows` <= rows_max rows of k (id, value) pairs; rank 0 receives world blocks of
 * rows_max rows each (short blocks padded with id -1 / value 0) in ids_root / vals_root. */
int pprhip_topk_gather(pprhip_comm_t* c, const int32_t* ids, const double* vals, int rows, int rows_max, int k,
                       int32_t* ids_root, double* vals_root);
/* Failure behaviour of the collectives.  A rank that fails inside pprhip_all_pair_backward_sharded before the
 * exchange still takes part in it with an error mark in its size words: every rank returns an error (the failing one
 * its own, the others PPRHIP_ERR_STATE "rank r failed before the exchange"), none blocks.  No wait on the fabric is
 * unbounded: after PPRHIP_COMM_TIMEOUT_S seconds (environment, default 1800) without completion, or when RCCL reports
 * an asynchronous error, the communicator is aborted (ncclCommAbort: peers' pending operations end with an error as
 * well) and every later collective on it fails at once.  A process that must leave a group early (its own failure
 * outside these calls) calls pprhip_comm_abort before pprhip_comm_destroy so that its peers are released.
 * (No reference counterpart: the Java is single-threaded, Gen_Util.java:208-232 / Base_Whole_Graph.java:76-92.) */
int pprhip_comm_abort(pprhip_comm_t* c);
/* The exchange's partition rule on the host (what k_owner_partition does to the device records): counts_out[world] =
 * entries whose source each rank owns, order_out[count] = the entries' indices owner by owner (stable).  With
 * pprhip_index_from_entries it lets a caller (the CPU multi-process tests, a host-side transport) carry the sharded
 * All-Pair over a fabric of its own with the library's own rule and finalisation (Base_Whole_Graph.java:84-86). */
int pprhip_owner_partition(uint32_t n, int world, const int32_t* sources, uint64_t count, uint64_t* counts_out,
                           uint64_t* order_out);
/* The finished index (k rule of Base_Whole_Graph.java:112-163 applied per source) from `count` entries
 * pi(sources[i], targets[i]) = values[i] in any order; ids are validated against [0, n). */
int pprhip_index_from_entries(uint32_t n, const int32_t* sources, const int32_t* targets, const double* values,
                              uint64_t count, int k, pprhip_index_t** index_out);

/* ---------------------------------------------------------------- single pairs (beyond the reference)
 * pi(s, t) for many pairs at once: the bidirectional estimator (BiPPR) built from a backward push from t and walks from
 * s.  pi is the vector pprhip_power_method(s, alpha, inf) and FORA estimate (a walk stops at a dead end with probability
 * alpha and otherwise restarts at s).  The push estimates the leaking PPR pi' (a dead end's (1 - alpha) mass is lost),
 * and pi(s, .) = pi'(s, .) / S(s) with S(u) the survival of a leaking walk from u (DESIGN.md §2 "Single pairs"), so
 *     value(s, t) = p_t(s) / S(s) + (1 / w) * sum_{i < w} r_t(V_i)
 * with p_t / r_t the reserve / residue of a backward push from t at r_max that starts r(t) = 1 and pops t (also when t
 * has no in-edges: p_t(t) = alpha, no residue - not Backward_Search.java:46-49's reserve(t) = 1), V_i the terminal of
 * walk i = (seed, PPRHIP_PAIR_WALK_STREAM, s, i) of pprhip_random_walk_batch (no_zero_hop = 0), and
 * w = ceil(omega * r_max), omega = 3 ln(2 / pfail) / (eps^2 delta): |value - pi| <= eps * max(pi, delta) with
 * probability >= 1 - pfail (delta, pfail from conf).  A pair's value depends on the seed and the pair only.
 * The push of a pair call runs under the handle's tuning (pprhip_graph_set_tuning): pprhip_backward_push under the
 * same tuning yields the same p_t and r_t up to fp64 addition order (when t has in-edges).  alpha, eps and rmax are
 * checked first (header "Parameter ranges"; rmax: 0 = the default below, else finite and 0 < rmax <= 1), then every
 * id before any device work (PPRHIP_ERR_INVALID, the handle untouched); q == 0 is an empty call; while a query stream
 * is open: PPRHIP_ERR_STATE.  After a pair call pprhip_get_reserve / _get_residue are undefined. */
#define PPRHIP_PAIR_WALK_STREAM 0xFFFFu /* the walk stream of every pair walk; no other path uses it */
/* Pure: r_max (rmax_in = 0: the balanced default eps * sqrt(dbar * delta / (3 ln(2 / pfail))), dbar = m / n, clamped
 * to (0, 1]) and the walks per pair w = ceil(omega * r_max) (at most 2^48). */
int pprhip_pair_params(const pprhip_fora_conf_t* conf, double eps, double rmax_in, double* rmax_out, uint64_t* walks_out);
/* S of the leaking walk at alpha, n doubles in original id order: S(u) = alpha + (1 - alpha) / d(u) * sum_{u->v} S(v)
 * for d(u) > 0, alpha at dead ends (1 on a graph without dead ends).  Jacobi iterations on the device until
 * (1 - alpha) / alpha * max|dS| <= 1e-14; computed once per (handle, alpha) and kept on the handle (8n bytes).
 * survival_out may be NULL (computes and keeps it). */
int pprhip_walk_survival(pprhip_graph_t* g, double alpha, double* survival_out);
/* q pairs (sources[i], targets[i]); values_out[i] = the estimate of pair i.  The pairs are grouped by target; every
 * distinct target is one backward push of a batched call (up to PPRHIP_BATCH in flight, their dense levels sharing
 * the batched sweeps), followed by the walks of its sources.  stats_sum: rmax_final = r_max, omega = omega,
 * walks / walk_steps / pops / edge_pushes / levels summed; push_ms / mc_ms: HIP-event times of the targets' push and
 * walk phases, summed over targets (they overlap); total_ms: the call. */
int pprhip_ppr_pairs(pprhip_graph_t* g, const int32_t* sources, const int32_t* targets, int q, double eps,
                     const pprhip_fora_conf_t* conf, double rmax, uint64_t seed, double* values_out,
                     pprhip_stats_t* stats_sum);

/* ---------------------------------------------------------------- single targets (beyond the reference)
 * The other direction as a query: which sources s rank a target t highly ("who reaches t": reverse recommendation,
 * audience, influence), for many targets and weighted target sets per call.  For a target set T with weights w (finite
 * values >= 0, NOT normalized; weights NULL: every w_t = 1, so that pi(s, T) is the probability that the walk from s
 * ends in T):
 *     value(s) ~ pi(s, T) = sum_t w_t pi(s, t)            for every source s,
 * with pi the engine's restarting PPR - the pi of pprhip_power_method, FORA and the pair call.  Estimator: a backward
 * push at threshold rmax from r = w (duplicates in a set summed, zero weights dropped), by the backward kernels and the
 * push test of pprhip_backward_push under the handle's tuning (pprhip_graph_set_tuning); then
 *     value(s) = p(s) / S(s),   S = pprhip_walk_survival(alpha)
 * (p the push's reserve; DESIGN.md §2 "Single targets").  A member whose weight does not pass the push test (w <= rmax)
 * starts as residue; a member without in-edges has nobody to push to and takes p = alpha * w at once.  A single target
 * (a set of one with weight 1) starts exactly as the pair call's push: r(t) = 1 and t is popped, also without in-edges
 * (p(t) = alpha, no residue - not Backward_Search.java:46-49's reserve(t) = 1).  So for a target with in-edges
 * value * S equals pprhip_backward_push's reserve under the same tuning, up to fp64 addition order.
 * Guarantee: the push invariant pi'(s, t) = p_t(s) + sum_v pi'(s, v) r_t(v) of the leaking PPR pi' is linear in the
 * start, after the push every residue is at most rmax, and sum_v pi'(s, v) = S(s); dividing by S(s):
 *     0 <= pi(s, T) - value(s) <= rmax       for every s.
 * The bound is deterministic: no walks, no seed.  A caller who wants relative error eps on values >= delta passes
 * rmax = eps * delta.  Top-k ranks by the lower bound `value`: it is not an exact top-k of pi (two sources whose
 * values differ by less than rmax may be swapped).
 * Checks, in this order and before any device work (PPRHIP_ERR_INVALID, the handle and a result on it untouched):
 * alpha ("Parameter ranges"), rmax finite with 0 < rmax <= 1; then q >= 0, k >= 0 and the buffers k asks for, the
 * store, offsets[0] == 0 and non-decreasing offsets; then per set, by the seed-set rules, with the set named in the
 * message (", set i: "): at least one member, every id in [0, n), every weight finite and >= 0, a weight sum > 0.
 * q == 0 is an empty call; while a query stream is open: PPRHIP_ERR_STATE.  After the call pprhip_get_reserve /
 * _get_residue are undefined, as after a pair call. */
/* q target sets described like the seed sets of pprhip_fora_batch_seeds: set i = targets / weights [offsets[i],
 * offsets[i + 1]); offsets NULL: q single targets, set i = {targets[i]} (weights NULL or q of them).  Up to
 * PPRHIP_BATCH sets are in flight on the handle's batch workspaces, their dense levels sharing the batched sweeps.
 * keep / values_out (q*n, query-major, original ids) / k / ids_out / vals_out / n_out / per_query / stats_sum as in
 * pprhip_fora_batch_single_source_resident; the top-k is selected over the scaled vector `value` by Algo_Util.kth_ppr's
 * rule (rows padded with -1 / 0; n_out may exceed k on ties).  Stats: the push counters (pops, edge_pushes, levels,
 * dense_levels), push_ms (host wall time of a set's push on its workspace, shared sweeps included; summed over sets in
 * stats_sum: they overlap), rmax_final = rmax and rounds = 1 per set; no walk field is set. */
int pprhip_ppr_targets(pprhip_graph_t* g, const int32_t* targets, const double* weights,
                       const uint64_t* offsets /* q+1, or NULL: q single targets */, int q, double alpha, double rmax,
                       pprhip_results_t* keep, double* values_out /* q*n or NULL */, int k, int32_t* ids_out,
                       double* vals_out, int* n_out, pprhip_stats_t* per_query, pprhip_stats_t* stats_sum);

/* ---------------------------------------------------------------- walk index (FORA+; beyond the reference)
 * FORA as published has a second form, FORA+: the terminals of walks drawn once are kept per node and a query reads
 * them instead of walking.  Here walk (seed, stream, start, walk_idx) is a pure function and every whole-graph FORA
 * path - pprhip_fora_single_source, pprhip_fora_seeds, the batched calls, the resident store, the query stream,
 * pprhip_fora_batch - draws the walks (seed, stream 0, v, 0 .. omega_v - 1) with the forced first hop for a residue
 * node v, whatever the query's source (a walk restarts at its own start node at a dead end).  An index that holds, for
 * node v, the terminals of the walks 0 .. cap(v) - 1 at one (alpha, seed) therefore serves such a query with the walks
 * it would have drawn itself: the result is the same vector up to fp64 addition order.
 * Use rule: a whole-graph FORA walk phase on a handle whose index was built at the call's alpha and seed (bit for bit)
 * reads walk i of residue node v from the index when i < cap(v) and walks it live, with its own index i, otherwise; with
 * another alpha or seed, or without an index, the phase runs as before.  Top-k rounds, pprhip_monte_carlo, the pair
 * walks and pprhip_random_walk_batch never touch the index.  Statistics of a served phase: walks and mc_sources as
 * without the index; walk_steps, walk_loads and walk_load_lanes count the live walks only.
 * Capacity: a converged push at threshold rmax leaves r(v) < d(v) * rmax, so node v starts at most
 * ceil(d(v) * (1 - alpha) * rmax * omega) walks: cap(v) = ceil(d(v) * density) with the density below covers every
 * query whose last threshold is <= rmax (a last round the cost model cut short may overflow; those walks are walked). */
/* While a query stream is open on the handle, _build, _drop, _fetch and _usage return PPRHIP_ERR_STATE like every other
 * call (_info does not touch the device and answers): usage is read after the stream's close. */
/* Pure: density = (1 - alpha) * rmax * omega * (1 + 2^-20) for conf and eps (pprhip_fora_whole_params); rmax == 0 means
 * rmax0, else finite and > 0.  The 2^-20 guard keeps rounding in d * density from leaving a converged push a terminal
 * short. */
int pprhip_walk_index_density(const pprhip_fora_conf_t* conf, double eps, double rmax, double* density_out);
/* Builds the index of (alpha, seed) on the handle: cap(v) = ceil(d_out(v) * density) terminals per node (none for a
 * dead end), terminal j of node v = the terminal of pprhip_random_walk_batch(start = v, walk_idx = j, alpha, seed,
 * stream = 0, no_zero_hop = 1).  density: finite and > 0, the total below 2^36 terminals (PPRHIP_ERR_INVALID
 * otherwise).  It lives with the lifted graph - every batch workspace and stream slot of the handle reads it - and is
 * read-only after the build; a second build replaces the first.  PPRHIP_ERR_OOM leaves the handle as it was; while a
 * query stream is open: PPRHIP_ERR_STATE.  stats (may be NULL): walks, walk_steps, mc_ms of the build. */
int pprhip_walk_index_build(pprhip_graph_t* g, double alpha, uint64_t seed, double density, pprhip_stats_t* stats);
/* Frees the index (no-op without one); pprhip_graph_release(PPRHIP_RELEASE_WALK_INDEX) does the same and
 * pprhip_graph_destroy frees it too. */
int pprhip_walk_index_drop(pprhip_graph_t* g);
/* What the handle's index holds (every output may be NULL; *present == 0: the others are zero). */
int pprhip_walk_index_info(const pprhip_graph_t* g, int* present, double* alpha, uint64_t* seed, double* density,
                           uint64_t* terminals, uint64_t* bytes);
/* The terminals of one node in original ids: *count_out = cap(node), the first min(cap, count) of them written. */
int pprhip_walk_index_fetch(pprhip_graph_t* g, int32_t node, int32_t* terminals_out, uint64_t cap, uint64_t* count_out);
/* Walks of the whole-graph FORA phases since the build (or the last reset) that were read from the index (served),
 * and walks of those phases that were walked live (walked: indices beyond a node's capacity, dead-end starts).  A phase
 * that did not use the index (other alpha or seed) counts in neither.  Covers the whole handle, batched calls
 * included; to be read when no call is in flight.  reset != 0 zeroes both afterwards. */
int pprhip_walk_index_usage(pprhip_graph_t* g, uint64_t* served, uint64_t* walked, int reset);
/* The single and the batch profile for a handle with an index.  They equal pprhip_tuning_default / pprhip_tuning_batch:
 * with c_walk_ns at the measured cost of a served walk the served runs were slower (DESIGN.md 2 "Walk index" has the
 * figures).  Nothing selects them implicitly: the caller sets them (pprhip_graph_set_tuning). */
void pprhip_tuning_indexed(pprhip_tuning_t* t);
void pprhip_tuning_indexed_batch(pprhip_tuning_t* t);

/* ---------------------------------------------------------------- local clustering (beyond the reference)
 * The sweep cut of PageRank-Nibble (Andersen, Chung, Lang) over a PPR vector, on the device: order the support by
 * x(v) / deg(v) and return the prefix of least conductance - "the cluster around these nodes".  The graph is read as
 * undirected; every relationship counts once whatever its direction, parallel relationships count each:
 *   deg(v) = d_out(v) + d_in(v) (a self loop adds 2); vol(S) = sum of deg over S, the total volume is 2m;
 *   cut(S) = relationships (a -> b), a != b, with exactly one endpoint in S (self loops never cut);
 *   phi(S) = cut(S) / min(vol(S), 2m - vol(S)), the fp64 quotient of the two integers; a prefix whose denominator is
 *   0 is not a candidate.
 * The input x is the result vector currently in HBM - what pprhip_get_reserve returns and pprhip_topk_select reads.
 * Node v is ranked when x(v) > 0 and deg(v) > 0.  Score: x(v) / (double)deg(v) with normalize = 1, x(v) with
 * normalize = 0.  Order: score descending, ties by original id ascending; position i is 0-based, prefix i is the
 * positions 0..i; vol[i] / cut[i] are those of prefix i (64-bit).  Best prefix: the candidate of smallest phi, ties to
 * the shortest; max_size > 0 admits prefixes of at most max_size nodes (and ends the profile there), max_vol > 0 those
 * with vol[i] <= max_vol.  Without a candidate: best_size = best_cut = best_vol = 0, best_conductance = +inf.
 * order_out / vol_out / cut_out receive the first min(cap, profiled) positions (ids are original ids); each may be
 * NULL, all must be NULL when cap == 0; info is required.  normalize outside {0, 1}, a null info and a buffer with
 * cap == 0 are PPRHIP_ERR_INVALID, checked before the handle; while a query stream is open: PPRHIP_ERR_STATE.  The
 * vector is not modified.  The workspace (76 bytes per node) is allocated by the handle's first sweep and kept:
 * pprhip_graph_release(PPRHIP_RELEASE_SWEEP) and pprhip_graph_destroy free it.  Every sum is an integer: the same
 * result every run. */
typedef struct pprhip_sweep {
  uint64_t support;      /* ranked nodes */
  uint64_t profiled;     /* prefixes whose vol / cut were computed (== support unless cut short by max_size) */
  uint64_t best_size, best_cut, best_vol;
  double best_conductance;
  uint64_t total_vol;    /* 2m */
  uint64_t edge_slots;   /* adjacency entries scanned (sum of deg over the profiled nodes) */
  double sort_ms, scan_ms, total_ms;  /* HIP-event times: support and order (with the count's read-back); the edge
                                       * scan kernel; the whole sweep up to the best prefix */
} pprhip_sweep_t;

/* over the vector pprhip_get_reserve would return */
int pprhip_sweep_cut(pprhip_graph_t* g, int normalize, uint64_t max_size, uint64_t max_vol,
                     int32_t* order_out, uint64_t* vol_out, uint64_t* cut_out, uint64_t cap, pprhip_sweep_t* info);
/* the same over vector i of a device-resident store (after pprhip_fora_batch_*_resident / _batch_seeds with keep) */
int pprhip_results_sweep_cut(pprhip_results_t* r, int i, int normalize, uint64_t max_size, uint64_t max_vol,
                             int32_t* order_out, uint64_t* vol_out, uint64_t* cut_out, uint64_t cap, pprhip_sweep_t* info);
/* PageRank-Nibble in one call: pprhip_forward_push_seeds(seeds, weights, alpha, rmax) with its outputs left in HBM,
 * then the sweep; members_out: the first min(cap, best_size) nodes of the order (the cluster).  alpha, rmax and the seed
 * set are checked by that call's rules (a bad set leaves the handle untouched); push_stats may be NULL. */
int pprhip_local_cluster_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double alpha,
                               double rmax, int normalize, uint64_t max_size, uint64_t max_vol, int32_t* members_out,
                               uint64_t cap, pprhip_sweep_t* info, pprhip_stats_t* push_stats);

/* ---------------------------------------------------------------- weighted relationships (beyond the reference)
 * Neo4j's PageRank takes a relationshipWeightProperty; the reference reads relationships as present or absent.  With
 * weights on the handle the pprhip_weighted_* calls below run over the transition matrix
 *   P(u, v) = sum of w(u -> v) / W(u),   W(u) = the sum of u's out-weights,
 * and compute the restarting pi of pprhip_power_method with this P: the walk stops with probability alpha per step and
 * jumps back to its start at a dead end.  Both directions exist: forward (power method, forward push, walks, whole-graph
 * FORA from one source) and backward (backward push, the survival vector, single targets / target sets, single pairs).
 * Only the pprhip_weighted_* calls read the weights.  Every entry point without that prefix ignores them - the
 * unweighted pprhip_backward_push, pprhip_ppr_targets and pprhip_ppr_pairs included - and so do the features that have
 * no weighted form: the query streams and the multi-GPU calls; they give what they gave before
 * pprhip_graph_set_weights.  pprhip_sweep_cut ranks by the relationship count whatever the weights are; the sweep by
 * weighted degree is pprhip_weighted_sweep_cut ("weighted local clustering" below).
 *
 * Weights: m doubles aligned with the out_col_idx given to pprhip_graph_create, every one finite and > 0 (a caller
 * drops relationships of weight <= 0 before the lift, so dead ends are exactly the unweighted dead ends), every row sum
 * finite.  A violation is PPRHIP_ERR_INVALID (the message names the edge index or the node), the handle and earlier
 * weights untouched; PPRHIP_ERR_OOM leaves the handle as it was; while a query stream is open: PPRHIP_ERR_STATE.  A
 * second call replaces the first; weights = NULL drops them.  pprhip_graph_release(PPRHIP_RELEASE_WEIGHTS) and
 * pprhip_graph_destroy free them.  HBM: out-weights, their per-row prefix and the in-row copy of the weights, 8 bytes
 * per edge each, and W per node: 24 m + 8 n bytes (R-MAT 22: 1.6 GB).
 * The prefix is part of the contract (walks are reproducible off the device): cum of a row is the left-to-right
 * sequential fp64 sum in row order, W its last element.  pprhip_weight_table_host is that rule and the same validation
 * as a pure host function, in the caller's order (cum_out: m doubles, wsum_out: n doubles; either may be NULL).
 *
 * Push: popping u with residue r credits reserve(u) += alpha r and deposits c w(e) along every out-edge, c =
 * (1 - alpha) r / W(u); a dead end returns (1 - alpha) r to the source as pprhip_forward_push does.  The push test is
 * the unweighted one, r / (double)d_out >= rmax with the relationship COUNT: a pop costs d_out edge visits whatever the
 * weights are, the test does not depend on the scale of the weights, and rsum <= rmax m, the walk budget,
 * pprhip_fora_whole_params and pprhip_walk_index_density hold unchanged.  Schedule: plain
 * frontier-synchronous Jacobi levels (every node active at level start pops from the level-start residues); the
 * tuning's gs_blocks / gs_frac are ignored, dense_frac only picks the kernel of a level.
 * Walk (seed, stream, start, idx): pprhip_random_walk_batch's function - same Philox key and counter, same words, stop
 * test, forced first hop, dead-end restart and step count - with the neighbour pick x = ((double)word * 2^-32) * W(cur),
 * j = the number of entries of the row's prefix that are <= x, clamped to d - 1, next = out_col_idx[row + j].
 *
 * Checks: the numeric parameters first ("Parameter ranges"), then the handle, then PPRHIP_ERR_STATE when the handle has
 * no weights.  Results stay in HBM as after the unweighted calls: pprhip_get_reserve / _residue, the sparse getters,
 * pprhip_topk_select and pprhip_sweep_cut work on them. */
/* (32u and 64u stay unassigned: the release tests of the handle use them as the flags nobody knows) */
#define PPRHIP_RELEASE_WEIGHTS 128u /* the relationship weights (pprhip_graph_set_weights): as set_weights(g, NULL) */
int pprhip_graph_set_weights(pprhip_graph_t* g, const double* weights /* m, or NULL: drop */);
int pprhip_weights_info(const pprhip_graph_t* g, int* present, uint64_t* bytes);
int pprhip_weight_table_host(uint32_t n, uint64_t m, const uint32_t* out_row_ptr, const double* weights,
                             double* cum_out, double* wsum_out);
/* the contract of pprhip_power_method */
int pprhip_weighted_power_method(pprhip_graph_t* g, int32_t src, double alpha, int iters, double* reserve_out,
                                 pprhip_stats_t* stats);
/* the contract of pprhip_forward_push */
int pprhip_weighted_forward_push(pprhip_graph_t* g, int32_t src, double alpha, double rmax, double* reserve_out,
                                 double* residue_out, double* rsum_out, pprhip_stats_t* stats);
/* the contract of pprhip_random_walk_batch */
int pprhip_weighted_random_walk_batch(pprhip_graph_t* g, const int32_t* starts, const uint64_t* walk_idx, uint64_t count,
                                      double alpha, uint64_t seed, uint32_t stream, int no_zero_hop,
                                      int32_t* terminals_out, uint32_t* steps_out /* may be NULL */);
/* One weighted push at rmax (0: rmax0 of pprhip_fora_whole_params), run to its end, then the walk phase of the
 * unweighted whole-graph FORA with weighted walks: rsum = (1 - alpha) * the residue sum, nrw = (long long)(omega rsum);
 * a residue entry r credits alpha r to its own reserve and starts omega_i = ceil(x) walks, x = (1 - alpha) r / rsum * nrw,
 * each adding (x / omega_i) / nrw * rsum at its terminal; walks (seed, stream 0, node, j < omega_i), forced first hop.
 * No threshold rounds and no cost model (the tuning constants were fitted on the unweighted kernels): rounds = 1. */
int pprhip_weighted_fora(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                         double rmax, double* reserve_out, pprhip_stats_t* stats);

/* ---- weighted seed sets and top-k ("Weighted seed sets and top-k"): relationshipWeightProperty
 * and sourceNodes in one query, and the reference's own top-k query over the weights.
 * Seed set: seeds / weights / n_seeds exactly as pprhip_forward_push_seeds takes them - p = the weights over their sum
 * (NULL: uniform), duplicates summed, zero weights dropped, the same refusals and messages - and p resolved for the
 * dead-end seeds by the same closed form (with D = the weight of the dead-end seeds, mass x landing on p gives a live
 * seed i the residue x q_i, q_i = p_i / (1 - (1 - alpha) D), and a dead-end seed j the reserve x alpha p_j / (1 - (1 -
 * alpha) D)).  Nothing of this depends on the relationship weights: dead ends are the unweighted dead ends.
 * Seeded push: the plain Jacobi levels of pprhip_weighted_forward_push with one change - a level's dead-end mass x lands
 * on p instead of on the source, inside the same level: r(i) += x q_i for every live seed, tested with the same crossing
 * rule, and x e_j into the reserve of every dead-end seed.  The first frontier is the set of live seeds; they pop
 * unconditionally.  A set whose seeds are all dead ends leaves reserve = p and runs no push.  A set of one seed is
 * pprhip_weighted_forward_push(s): the same levels and pops, vectors equal up to the order of additions.
 * Top-k: Fora_Topk's schedule on delta, which does not depend on the weights - eps / 2, delta from conf->delta to
 * max(min_delta, delta / 4) per round, the loop ends when kth >= (1 + eps / 2) delta or delta <= min_delta - over plain
 * rounds.  Round j: rmax_j = the scaled push threshold of pprhip_fora_topk_params(delta), omega_j its omega; the first
 * frontier is the live seeds (j = 0) or every node with r / d_out >= rmax_j (j > 0; possibly none); the levels above run
 * at rmax_j to their end on the residues and the reserve the rounds before left; estimate := reserve; the walk plan of
 * pprhip_fora_topk (rsum = (1 - alpha) * the residue sum, nrw = (long long)(omega_j rsum), an entry r starts ceil(r nrw)
 * walks, each adding (r nrw / omega_i) / nrw); the walks are pprhip_weighted_random_walk_batch's (seed, stream j, node,
 * index) without the forced first hop; then the selection of k and its k-th value (0 when fewer than k are positive).
 * No parking or arming, no push ahead on a second stream, no cost model.  After every round no node is active at
 * rmax_j.  No live seed: the estimate is p, rounds = 0, one selection.  The result is left as pprhip_fora_topk leaves it
 * (pprhip_get_reserve, the sparse getters, pprhip_topk_select and pprhip_sweep_cut read the estimate); rows are padded
 * -1 / 0; the stats are filled as by pprhip_fora_topk (rounds, levels, dense_levels, pops, walks, walk_steps,
 * mc_sources, kth_value, rsum, rmax_final, omega, the times).
 * Checks, in this order: the numeric parameters (the top-k calls: a top-k conf), the handle (an open query stream:
 * PPRHIP_ERR_STATE), PPRHIP_ERR_STATE without weights, then ids and sets before any device work. */
/* the contract of pprhip_forward_push_seeds, with the seeded weighted push */
int pprhip_weighted_forward_push_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                                       double alpha, double rmax, double* reserve_out, double* residue_out,
                                       double* rsum_out, pprhip_stats_t* stats);
/* The seeded weighted push at rmax (0: rmax0), then pprhip_weighted_fora's walk phase unchanged: the whole-graph plan,
 * stream 0, forced first hop, a walk restarts at its own start node at a dead end, rounds = 1.  No live seed: the
 * estimate is p. */
int pprhip_weighted_fora_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds, double eps,
                               const pprhip_fora_conf_t* conf, uint64_t seed, double rmax, double* reserve_out,
                               pprhip_stats_t* stats);
/* signature and delivery of pprhip_fora_topk: the weighted top-k rounds from the set {src} with weight 1 */
int pprhip_weighted_fora_topk(pprhip_graph_t* g, int32_t src, double eps, const pprhip_fora_conf_t* conf, uint64_t seed,
                              int32_t* ids_out, double* vals_out, int cap, int* n_out, double* reserve_out,
                              pprhip_stats_t* stats);
/* signature and delivery of pprhip_fora_topk_seeds: the weighted top-k rounds from a seed set */
int pprhip_weighted_fora_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                                    double eps, const pprhip_fora_conf_t* conf, uint64_t seed, int32_t* ids_out,
                                    double* vals_out, int cap, int* n_out, double* reserve_out, pprhip_stats_t* stats);

/* ---- batched weighted FORA ("Batched weighted FORA"): q weighted whole-graph queries in one call,
 * up to 16 of them in flight on the handle's batch workspaces (PPRHIP_BATCH_WORKSPACES: fewer), their dense levels
 * sharing one sweep over the interleaved contributions.  Query i runs as pprhip_weighted_fora(srcs[i], eps, conf, seed,
 * rmax) / pprhip_weighted_fora_seeds(set i, ...) would: the same dense / sparse rule on its own frontier, the same
 * thresholds, the same walk plan, the same walks (every query walks with the call's seed, stream 0, forced first hop),
 * served from the weighted walk index where the single call is.  Batching changes the order of fp64 additions and
 * nothing else.  A dead-end source runs no push and no walks (reserve = e_s), a set without a live seed neither
 * (reserve = p).  Terminals are not shared between the queries of a call.
 * rmax (0: rmax0 of conf and eps) as in pprhip_weighted_fora; every other argument and output means what it means in
 * pprhip_fora_batch_single_source_resident / pprhip_fora_batch_seeds: keep (NULL: none) receives every vector,
 * reserve_out (NULL: none) q x n doubles, k > 0 the top-k of every vector (rows padded -1 / 0, n_out[i] as there),
 * per_query (NULL: none) q statistics as pprhip_weighted_fora fills them - levels, dense_levels, pops, dense_nodes,
 * edge_pushes, walks, walk_steps, dead_end_pops, rsum, rmax_final, omega, rounds = 1; push_ms and mc_ms on the host's
 * clock - and stats_sum their sums with the call's kernel classes (the sweeps are class PPRHIP_KERNEL_DENSE_PULL_BATCH).
 * Checks, in this order, all before anything runs: the numeric parameters (pprhip_weighted_fora's), the handle,
 * PPRHIP_ERR_STATE without weights, q / k / the top-k rows, keep, then every source / every set.  q = 0 is
 * PPRHIP_OK with keep->count = 0.  An error on any workspace ends the call; the handle stays usable. */
int pprhip_weighted_fora_batch(pprhip_graph_t* g, const int32_t* srcs, int q, double eps, const pprhip_fora_conf_t* conf,
                               uint64_t seed, double rmax, pprhip_results_t* keep, double* reserve_out, int k,
                               int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                               pprhip_stats_t* stats_sum);
/* ... over q seed sets described like a CSR (pprhip_fora_batch_seeds): set i = seeds / weights [offsets[i], offsets[i + 1]) */
int pprhip_weighted_fora_batch_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights,
                                     const uint64_t* offsets, int q, double eps, const pprhip_fora_conf_t* conf,
                                     uint64_t seed, double rmax, pprhip_results_t* keep, double* reserve_out, int k,
                                     int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                     pprhip_stats_t* stats_sum);

/* ---- batched weighted top-k ("Batched weighted top-k"): q weighted top-k queries in one call, up
 * to 16 of them in flight on the handle's batch workspaces (PPRHIP_BATCH_WORKSPACES: fewer; the first such call
 * allocates the batch state).  conf is a top-k conf (pprhip_conf_fora_topk), k is conf->k.  Query i IS
 * pprhip_weighted_fora_topk(srcs[i], eps, conf, seed + i, ...) / pprhip_weighted_fora_topk_seeds(set i, ..., seed + i,
 * ...): the same schedule on delta, the same rmax_j and omega_j per round, the same first frontier per round (the live
 * seeds, then every node active at rmax_j), the same dense / sparse rule on its own frontier, the same walk plan and the
 * same walks (seed + i, stream = round, node, index; no forced first hop), the same selection and the same stop rule;
 * no parking, no push ahead, no cost model.  Batching changes the order of fp64 additions (sweeps, terminal atomics) and
 * nothing else.  The dense levels of the queries in flight share the batched weighted sweep; a column at a dense level
 * never waits for another column.  The walk plans of all columns whose round has reached its walk phase run in ONE
 * launch, the waves dealt to the columns by their walk counts (pprhip_walk_multi_shares is the rule).  The weighted walk
 * index is never read.  A call with q == 1 runs the single call's loop on the handle's own workspace.
 * ids_out / vals_out: q x k, rows padded -1 / 0; n_out (NULL: none): q counts as the single call's n_out; keep (NULL:
 * none) receives query i's estimate vector - what pprhip_get_reserve returns after the single call - in slot i;
 * per_query (NULL: none): q statistics filled as the single call fills them (rounds, levels, dense_levels, pops,
 * dense_nodes, enqueues, walks, walk_steps, mc_sources, dead_end_pops, kth_value, rsum, rmax_final, omega.  push_ms,
 * mc_ms and select_ms are NOT the single call's event times: they are host times of the driver rounds the query took
 * part in - mc_ms the time to queue the round's walk plans, merged launch and selections, select_ms the wait for the
 * selection (the merged walk's device time and, for a later column, the deliveries of the columns before it fall into
 * it), push_ms the rest - and a phase shared with other columns is counted for each); stats_sum: their sums
 * and the call's kernel classes - the sweeps are class PPRHIP_KERNEL_DENSE_PULL_BATCH (busy columns per sweep =
 * dense_levels / class_launches[5]), the merged walk launches class PPRHIP_KERNEL_WALK (columns per launch = rounds /
 * class_launches[3]).  A dead-end source or a set without a live seed: rounds = 0, the estimate is p, one selection.
 * Checks, all before any device work: eps, the conf, q < 0 and NULL rows with q > 0 (PPRHIP_ERR_INVALID), then the
 * handle (an open query stream: PPRHIP_ERR_STATE), PPRHIP_ERR_STATE without weights, keep, then every source / every
 * set (the message names the set).  q = 0 is PPRHIP_OK with keep->count = 0 and zeroed stats_sum.  An error on any
 * workspace ends the call; the handle stays usable. */
int pprhip_weighted_fora_batch_topk(pprhip_graph_t* g, const int32_t* srcs, int q, double eps,
                                    const pprhip_fora_conf_t* conf, uint64_t seed, pprhip_results_t* keep,
                                    int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                    pprhip_stats_t* stats_sum);
/* ... over q seed sets described like a CSR (pprhip_fora_batch_seeds) */
int pprhip_weighted_fora_batch_topk_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights,
                                          const uint64_t* offsets, int q, double eps, const pprhip_fora_conf_t* conf,
                                          uint64_t seed, pprhip_results_t* keep, int32_t* ids_out, double* vals_out,
                                          int* n_out, pprhip_stats_t* per_query, pprhip_stats_t* stats_sum);
/* The dealing rule of the merged walk launch, without a device.  counts[c]: the walks of column c's plan (0: idle);
 * base_waves >= 1: the waves of a single walk launch.  T = the sum of the counts, per = ceil(ceil(T / 64) / base_waves)
 * * 64 (0 when T is 0); column c owns the ceil(counts[c] / per) consecutive waves from first_out[c], wave b of them runs
 * the column's walks [(b - first_out[c]) * per, min(.. + per, counts[c])); no wave spans two columns; first_out[16] =
 * the waves in use <= base_waves + 15, which is the grid the launch uses.  The launch's base_waves is n_cus * 16: a top-k
 * plan derives its walk budget on the device, so the host has no bound of the walk count to trim the grid by. */
int pprhip_walk_multi_shares(const uint64_t counts[16], uint32_t base_waves, uint64_t* per_out, uint32_t first_out[17]);

/* ---- weighted walk index (FORA+ for pprhip_weighted_fora and pprhip_weighted_fora_seeds; DESIGN.md section 2,
 * "Weighted walk index"): the walk index above, over the weighted walks.  Both weighted whole-graph calls plan with the
 * unweighted plan and draw the weighted walks (seed, stream 0, v, 0 .. omega_v - 1) with the forced first hop for a
 * residue node v; the weighted push test keeps the relationship count, so cap(v) = ceil(d_out(v) * density) with
 * pprhip_walk_index_density's density covers every such call whose threshold is <= rmax, as it does unweighted.
 * Terminal j of node v = the terminal of pprhip_weighted_random_walk_batch(start = v, walk_idx = j, alpha, seed,
 * stream = 0, no_zero_hop = 1).
 * Use rule: the walk phase of pprhip_weighted_fora / pprhip_weighted_fora_seeds on a handle whose weighted index was
 * built at the call's alpha (bit for bit) and seed reads walk i of residue node v from it when i < cap(v) and walks it
 * live, with its own index i, otherwise (every walk of a dead-end start is walked: its capacity is 0); the result is
 * the same vector up to fp64 addition order.  With another alpha or seed, or without the index, the phase runs as
 * before.  The weighted top-k rounds, pprhip_weighted_ppr_pairs and pprhip_weighted_random_walk_batch never touch it.
 * Statistics of a served phase: walks and mc_sources as without the index, walk_steps counts the live walks only.
 * The two indexes coexist on a handle and neither is ever read by the other family of calls:
 * PPRHIP_RELEASE_WALK_INDEX and pprhip_walk_index_drop leave the weighted index alone.  It is built from the weights:
 * pprhip_graph_set_weights (new weights or NULL) and pprhip_graph_release(PPRHIP_RELEASE_WEIGHTS) drop it before the
 * weights change (a refused pprhip_graph_set_weights changes nothing and leaves it); pprhip_graph_destroy frees it.
 * The five calls take the arguments of their unweighted namesakes, check them in the same order with the same
 * messages under their own names, and fill the same statistics; _build returns PPRHIP_ERR_STATE on a handle without
 * weights (after the checks of the numbers and of the handle). */
#define PPRHIP_RELEASE_WEIGHTED_WALK_INDEX 256u /* the weighted walk index: as pprhip_weighted_walk_index_drop */
int pprhip_weighted_walk_index_build(pprhip_graph_t* g, double alpha, uint64_t seed, double density,
                                     pprhip_stats_t* stats);
int pprhip_weighted_walk_index_drop(pprhip_graph_t* g);
int pprhip_weighted_walk_index_info(const pprhip_graph_t* g, int* present, double* alpha, uint64_t* seed,
                                    double* density, uint64_t* terminals, uint64_t* bytes);
int pprhip_weighted_walk_index_fetch(pprhip_graph_t* g, int32_t node, int32_t* terminals_out, uint64_t cap,
                                     uint64_t* count_out);
int pprhip_weighted_walk_index_usage(pprhip_graph_t* g, uint64_t* served, uint64_t* walked, int reset);

/* ---- the backward direction over the same P ("Weighted backward direction")
 * Backward push: popping v with residue r credits reserve(v) += alpha r and deposits (c w(e)) / W(u) on r(u) along every
 * in-edge e = (u -> v), c = (1 - alpha) r; with every weight equal to one power of two that is bit for bit the
 * unweighted c / d_out(u).  u joins the next level when its residue crosses the unweighted backward test
 * !(old > rmax) && new > rmax - strict, un-normalised, no degree in it, so nothing about it changes with the weights.
 * Schedule: plain frontier-synchronous Jacobi levels; gs_blocks / gs_frac are ignored, dense_frac only picks the kernel
 * of a level (sparse: one atomic per in-edge; dense: a pull over the out-rows, summed per row and divided by W once).
 * Survival: S_w(u) = alpha + (1 - alpha) / W(u) * sum_{u -> v} w(u -> v) S_w(v), alpha at dead ends, by Jacobi from alpha
 * until (1 - alpha) / alpha * max|dS| <= 1e-14; kept on the handle per alpha beside the unweighted S, freed with the
 * weights (pprhip_graph_set_weights, also with NULL; PPRHIP_RELEASE_WEIGHTS; pprhip_graph_destroy).
 * Targets: value(s) = p(s) / S_w(s) with 0 <= pi(s, T) - value(s) <= rmax, pi the restarting PPR over P.
 * Pairs: value(s, t) = p_t(s) / S_w(s) + (1 / w) sum_{i < w} r_t(V_i), V_i the terminal of the weighted walk (seed,
 * PPRHIP_PAIR_WALK_STREAM, s, i) without the forced first hop - pprhip_weighted_random_walk_batch's function; r_max and
 * w are pprhip_pair_params', unchanged.  A pair's walk sums are formed without atomics in a fixed order.
 * A target call of q >= 2 queries runs with up to PPRHIP_BATCH of them in flight on the handle's batch workspaces, the
 * queries that stand at a dense level sharing one 16-column sweep over the out-rows; it allocates the batch state on
 * first use, as pprhip_ppr_targets does (PPRHIP_RELEASE_BATCH hands it back; PPRHIP_BATCH_WORKSPACES limits the
 * columns).  Query i takes, level by level, the decisions of the call of that one query - the same dense / sparse rule
 * on its own frontier, the same threshold test, the same start rules - and batching changes the order of additions
 * inside dense levels only; per-query push_ms / total_ms are the host's clock, stats_sum carries the call's kernel
 * classes (class_launches[PPRHIP_KERNEL_DENSE_PULL_BATCH]: the shared sweeps).  A call of q == 1 and the pairs'
 * distinct targets run one after another on the handle's own workspace and allocate no batch state.
 * Checks as above: parameter ranges, the handle (an open query stream:
 * PPRHIP_ERR_STATE), PPRHIP_ERR_STATE without weights, then ids and sets before any device work, the handle untouched. */
/* the contract of pprhip_backward_push (in-degree 0: reserve(t) = 1 and no push); results stay in HBM for the getters,
 * the sparse getters, pprhip_topk_select and pprhip_sweep_cut */
int pprhip_weighted_backward_push(pprhip_graph_t* g, int32_t target, double alpha, double rmax, double* reserve_out,
                                  double* residue_out, pprhip_stats_t* stats);
/* the contract of pprhip_walk_survival */
int pprhip_weighted_walk_survival(pprhip_graph_t* g, double alpha, double* survival_out /* may be NULL */);
/* signature, checks, start rules (single target: r(t) = 1 and t pops, p(t) = alpha without in-edges; a set starts from
 * r = w), delivery (keep, values_out, top-k rows padded -1 / 0) and stats of pprhip_ppr_targets; pprhip_get_reserve /
 * _residue are undefined afterwards */
int pprhip_weighted_ppr_targets(pprhip_graph_t* g, const int32_t* targets, const double* weights, const uint64_t* offsets,
                                int q, double alpha, double rmax, pprhip_results_t* keep, double* values_out, int k,
                                int32_t* ids_out, double* vals_out, int* n_out, pprhip_stats_t* per_query,
                                pprhip_stats_t* stats_sum);
/* signature, checks and stats of pprhip_ppr_pairs; a target without in-edges is exact and walks nothing */
int pprhip_weighted_ppr_pairs(pprhip_graph_t* g, const int32_t* sources, const int32_t* targets, int q, double eps,
                              const pprhip_fora_conf_t* conf, double rmax, uint64_t seed, double* values_out,
                              pprhip_stats_t* stats_sum);

/* ---- All-Pair backward search over the same P ("Weighted All-Pair")
 * pprhip_all_pair_backward's index over the weighted transition matrix: signature, k rule, target ranges, the
 * index type (pprhip_index_merge / _arrays / _write_dir work on it unchanged) and the meaning of every stats field are
 * the unweighted call's.  One search per target t is the frontier-synchronous weighted backward push with the start rule
 * of pprhip_weighted_backward_push at rmax = threshold: t pops first whatever the threshold; a popped v credits alpha r
 * to its reserve and holds c = (1 - alpha) r; every in-edge e = (u -> v) deposits c * p(e) on r(u), p(e) = w(e) / W(u)
 * rounded ONCE when the edge records are built; u joins the next level iff !(old > threshold) && new > threshold; a
 * target without in-edges yields {t: 1.0}; entries with reserve > 0 and reserve >= threshold are emitted.  A deposit
 * c * (w / W) may differ by an ulp from pprhip_weighted_backward_push's (c * w) / W; with power-of-two row sums both are
 * exact.  The searches that the table and dense tiers give up run as pprhip_weighted_backward_push's whole-vector search
 * (deposits (c * w) / W), one after another, whatever their number.
 * Checks: alpha, threshold, the handle, PPRHIP_ERR_STATE without weights, then the target range.
 * The edge records {source, p} (16 bytes per relationship) are built on the first call and kept beside the weights:
 * pprhip_weights_info counts them from then on; pprhip_graph_set_weights (also with NULL), PPRHIP_RELEASE_WEIGHTS and
 * PPRHIP_RELEASE_ALL_PAIR free them.  The workspaces are shared with pprhip_all_pair_backward; the two calls may be
 * interleaved on one handle.
 * Not offered over the weights: pprhip_all_pair_backward_multi / _sharded and the comm entry points (target ranges plus
 * pprhip_index_merge shard by hand), the ppr command line and the JNI binding. */
int pprhip_weighted_all_pair_backward(pprhip_graph_t* g, double alpha, double threshold, int k, uint32_t t_begin,
                                      uint32_t t_end, pprhip_index_t** index_out, pprhip_stats_t* stats);

/* ---- weighted local clustering ("Weighted sweep cut"): the sweep cut by relationship weight,
 * PageRank-Nibble on the weighted graph.  The graph is read as pprhip_sweep_cut reads it - undirected, a node's
 * adjacency its out-row followed by its in-row, every relationship once, parallel relationships each, a self loop never
 * cuts and adds its weight twice to the degree - and the order of the steps, the outputs and `cap` are that call's.
 * Quanta: the weights enter as integers in fixed point, so that every sum is a 64-bit integer and the result the same
 * words every run (sums of fp64 weights depend on the order of addition).  With wmax the largest of the m weights,
 * e the exponent of frexp(wmax) (wmax = f 2^e, 0.5 <= f < 1) and L the smallest integer with m <= 2^L, the shift is
 * s = 61 - e - L and the quantum of relationship e is q(e) = max(1, llrint(ldexp(w(e), s))), rounded to nearest, ties to
 * even: a weight below half a quantum counts as one quantum, no relationship vanishes.  q(e) <= 2^(61 - L), the sum of
 * all q <= 2^61, the total volume <= 2^62.  One weight unit is 2^s quanta.  The rule depends on wmax and m only.
 * pprhip_weight_quantum gives s for a weight array as a pure host function, with the validation of
 * pprhip_weight_table_host (a weight that is not finite and > 0 is PPRHIP_ERR_INVALID, the message names the edge);
 * weights may be NULL when m == 0, and s = 0 then.
 *   qdeg(v) = the sum of q over v's out-row plus its in-row; vol_q(S) = sum of qdeg over S; total_vol_q = 2 sum q;
 *   cut_q(S) = the sum of q over relationships (a -> b), a != b, with exactly one endpoint in S;
 *   phi(S) = (double)cut_q / (double)min(vol_q, total_vol_q - vol_q): two conversions uint64 -> fp64 to nearest and one
 *   division; a prefix whose denominator is 0 is not a candidate.
 * Node v is ranked when x(v) > 0 and it has at least one adjacency slot (then qdeg(v) >= 1).  Score: x(v) /
 * (double)qdeg(v) with normalize = 1, x(v) with normalize = 0; order: score descending, ties by original id ascending.
 * max_size as in pprhip_sweep_cut.  max_vol is a double in weight units, finite and >= 0, 0: no bound; a prefix is
 * admitted when vol_q <= min(2^63 - 1, floor(ldexp(max_vol, s))), a limit formed on the host.  Best prefix: the
 * smallest phi, ties to the shortest; without a candidate best_size = best_cut_q = best_vol_q = 0, best_conductance =
 * +inf.  The input is whatever result vector is in HBM, whichever call put it there; it is not modified.
 * Checks, in this order: normalize outside {0, 1}, a null info, a buffer with cap == 0, a max_vol that is negative, NaN
 * or infinite (the one-call form: then alpha and rmax) are PPRHIP_ERR_INVALID before the handle is looked at, the
 * message naming the entry point and the parameter; then the handle (an open query stream: PPRHIP_ERR_STATE); then
 * PPRHIP_ERR_STATE when the handle has no weights.
 * Memory: qdeg (8 n bytes), s and total_vol_q are built by the first weighted sweep after pprhip_graph_set_weights (one
 * pass over the 16 m bytes of the two weight arrays) and kept beside the weights: pprhip_weights_info counts the 8 n
 * bytes while they exist; pprhip_graph_set_weights (also with NULL), PPRHIP_RELEASE_WEIGHTS and pprhip_graph_destroy
 * free them.  The sweep workspace of pprhip_sweep_cut is shared; the first weighted sweep adds 8 (n + 1) bytes to it
 * (the volume in quanta), freed with it by PPRHIP_RELEASE_SWEEP and pprhip_graph_destroy.  Weighted and unweighted sweeps
 * may be interleaved on one handle; a handle that never runs a weighted sweep pays nothing. */
typedef struct pprhip_wsweep {
  uint64_t support;      /* ranked nodes */
  uint64_t profiled;     /* prefixes whose vol_q / cut_q were computed (== support unless cut short by max_size) */
  uint64_t best_size, best_cut_q, best_vol_q;  /* the best prefix, cut and volume in quanta */
  double best_conductance;
  uint64_t total_vol_q;  /* 2 sum q */
  int32_t shift;         /* s: one weight unit is 2^s quanta */
  int32_t reserved;
  uint64_t edge_slots;   /* adjacency entries scanned (the count, as in pprhip_sweep_t) */
  double sort_ms, scan_ms, total_ms;  /* as in pprhip_sweep_t; the one-off build of qdeg lies before total_ms begins */
} pprhip_wsweep_t;

int pprhip_weight_quantum(uint64_t m, const double* weights, int* shift_out);
/* over the vector pprhip_get_reserve would return; order_out / vol_q_out / cut_q_out and cap as in pprhip_sweep_cut */
int pprhip_weighted_sweep_cut(pprhip_graph_t* g, int normalize, uint64_t max_size, double max_vol, int32_t* order_out,
                              uint64_t* vol_q_out, uint64_t* cut_q_out, uint64_t cap, pprhip_wsweep_t* info);
/* the same over vector i of a device-resident store */
int pprhip_results_weighted_sweep_cut(pprhip_results_t* r, int i, int normalize, uint64_t max_size, double max_vol,
                                      int32_t* order_out, uint64_t* vol_q_out, uint64_t* cut_q_out, uint64_t cap,
                                      pprhip_wsweep_t* info);
/* pprhip_weighted_forward_push_seeds(seeds, weights, alpha, rmax) with its outputs left in HBM, then the weighted sweep:
 * the counterpart of pprhip_local_cluster_seeds.  members_out: the first min(cap, best_size) nodes of the order.  alpha,
 * rmax and the seed set follow that call's rules (a bad set leaves the handle untouched); push_stats may be NULL. */
int pprhip_weighted_local_cluster_seeds(pprhip_graph_t* g, const int32_t* seeds, const double* weights, int n_seeds,
                                        double alpha, double rmax, int normalize, uint64_t max_size, double max_vol,
                                        int32_t* members_out, uint64_t cap, pprhip_wsweep_t* info,
                                        pprhip_stats_t* push_stats);

/* ---------------------------------------------------------------- ground truth (a12) */
/* Power_Method.computeWholeGraphPPR (Power_Method.java:44-101): `iters` synchronous sweeps. */
int pprhip_power_method(pprhip_graph_t* g, int32_t src, double alpha, int iters, double* reserve_out,
                        pprhip_stats_t* stats);

#ifdef __cplusplus
}
#endif
#endif /* PPRHIP_H */
