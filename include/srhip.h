/*
 * srhip.h — C ABI of libsrhip.so, the MI355X (gfx950) batched expression-evaluation
 * engine for SymbolicRegression.jl's hot path (eval_tree_array -> _eval_loss -> score_func).
 *
 * Every entry point is plain C: opaque handles, plain pointers and sizes, integer status.
 * No C++ exception crosses this boundary.  `did_succeed == false` is DATA (out_ok[t] == 0),
 * not an error.  On a nonzero status, srhip_last_error() returns a thread-local message.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *   srhip_eval_loss        <- _eval_loss / eval_loss            src/LossFunctions.jl:45-75, 97-112
 *                             (batched over a population:       src/Population.jl:36-62,162-176,
 *                              src/SingleIteration.jl:64-82)
 *   srhip_eval_predict     <- eval_tree_array(tree, X, options) src/InterfaceDynamicExpressions.jl:56-63
 *                             (-> DynamicExpressions.eval_tree_array, external v0.16)
 *   srhip_dataset_create   <- Dataset{T,L}(X, y; weights)      src/Dataset.jl:98-225
 *   srhip_program_create   <- the Node{T} trees + options.operators (OperatorEnum)
 *                                                               src/Options.jl:92-150,673-681
 *   srhip_program_set_constants <- set_constants!/Optim's constant vector (constant optimizer)
 *                                                               src/ConstantOptimization.jl:43-81
 *   srhip_eval_loss_batch  <- score_func over many members (convenience: create+eval+destroy)
 *                                                               src/LossFunctions.jl:161-174
 */
#ifndef SRHIP_H
#define SRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
enum {
  SRHIP_OK = 0,
  SRHIP_ERR_INVALID = 1,     /* malformed argument (bad tree, out-of-range feature, ...) */
  SRHIP_ERR_UNSUPPORTED = 2, /* operator / dtype / loss the device does not implement,  */
                             /* or a tree needing > 8 interpreter stack slots           */
  SRHIP_ERR_DEVICE = 3,      /* HIP runtime error                                       */
  SRHIP_ERR_NOMEM = 4
};

/* ---- element types (Dataset{T}) --------------------------------------------------------- */
enum { SRHIP_F32 = 0, SRHIP_F64 = 1, SRHIP_I32 = 2 };

/* ---- operator codes: the device's op table (reference src/Operators.jl + Julia Base).
 * options.operators.binops[i] / unaops[i] (1-based op index stored in Node.op) are mapped to
 * these codes by the host binding (Julia glue / Python mirror), after the reference's own
 * aliasing binopmap/unaopmap (src/Options.jl:92-150): ^ -> safe_pow, log -> safe_log, ...    */
enum {
  /* binary */
  SRHIP_OP_ADD = 1, SRHIP_OP_SUB = 2, SRHIP_OP_MUL = 3, SRHIP_OP_DIV = 4,
  SRHIP_OP_POW = 5,         /* safe_pow   src/Operators.jl:28-36 */
  SRHIP_OP_GREATER = 6,     /* greater    src/Operators.jl:82-84 */
  SRHIP_OP_COND = 7,        /* cond       src/Operators.jl:85-87 */
  SRHIP_OP_LOGICAL_OR = 8,  /* src/Operators.jl:91-93 */
  SRHIP_OP_LOGICAL_AND = 9, /* src/Operators.jl:94-96 */
  SRHIP_OP_MAX = 10, SRHIP_OP_MIN = 11, /* Julia Base max/min (NaN-propagating) */
  SRHIP_OP_MOD = 12,        /* Julia Base mod (floored, sign of divisor) */
  SRHIP_OP_ATAN2 = 13,      /* Julia Base atan(y, x) */
  /* unary */
  SRHIP_OP_NEG = 32, SRHIP_OP_SQUARE = 33, SRHIP_OP_CUBE = 34, SRHIP_OP_ABS = 35,
  SRHIP_OP_RELU = 36,       /* src/Operators.jl:88-90 (Bool strong zero) */
  SRHIP_OP_COS = 37, SRHIP_OP_SIN = 38, SRHIP_OP_TAN = 39, SRHIP_OP_EXP = 40,
  SRHIP_OP_LOG = 41,        /* safe_log   src/Operators.jl:37-40 */
  SRHIP_OP_LOG2 = 42, SRHIP_OP_LOG10 = 43, SRHIP_OP_LOG1P = 44,
  SRHIP_OP_SQRT = 45,       /* safe_sqrt  src/Operators.jl:57-60 */
  SRHIP_OP_ACOSH = 46,      /* safe_acosh src/Operators.jl:53-56 */
  SRHIP_OP_ATANH_CLIP = 47, /* atanh_clip src/Operators.jl:17   */
  SRHIP_OP_SINH = 48, SRHIP_OP_COSH = 49, SRHIP_OP_TANH = 50,
  SRHIP_OP_ASIN = 51, SRHIP_OP_ACOS = 52, SRHIP_OP_ATAN = 53, SRHIP_OP_ASINH = 54,
  SRHIP_OP_ERF = 55, SRHIP_OP_ERFC = 56,
  SRHIP_OP_GAMMA = 57,      /* gamma (Inf -> NaN) src/Operators.jl:11-15 */
  SRHIP_OP_ROUND = 58, SRHIP_OP_FLOOR = 59, SRHIP_OP_CEIL = 60, SRHIP_OP_SIGN = 61,
  SRHIP_OP_EXP2 = 62, SRHIP_OP_EXPM1 = 63, SRHIP_OP_CBRT = 64
};

/* ---- loss kinds (LossFunctions.jl 0.10/0.11 supervised losses; src/LossFunctions.jl:13-33,
 * the list src/Options.jl:209-229 documents).  Distance losses take r = output - target, margin
 * losses the agreement a = target * output (LossFunctions' MarginLoss convention). */
enum {
  SRHIP_LOSS_L2 = 0,          /* L2DistLoss (default, src/Options.jl:534-535) */
  SRHIP_LOSS_L1 = 1,          /* L1DistLoss */
  SRHIP_LOSS_LP = 2,          /* LPDistLoss{P}: p0 = P */
  SRHIP_LOSS_HUBER = 3,       /* HuberLoss(d): p0 = d */
  SRHIP_LOSS_L1_EPS_INS = 4,  /* L1EpsilonInsLoss(eps): p0 = eps */
  SRHIP_LOSS_L2_EPS_INS = 5,  /* L2EpsilonInsLoss(eps): p0 = eps */
  SRHIP_LOSS_LOGIT_DIST = 6,  /* LogitDistLoss */
  SRHIP_LOSS_PERIODIC = 7,    /* PeriodicLoss(c): p0 = c */
  SRHIP_LOSS_QUANTILE = 8,    /* QuantileLoss(tau): p0 = tau */
  SRHIP_LOSS_ZERO_ONE = 9,            /* ZeroOneLoss */
  SRHIP_LOSS_PERCEPTRON = 10,         /* PerceptronLoss */
  SRHIP_LOSS_LOGIT_MARGIN = 11,       /* LogitMarginLoss */
  SRHIP_LOSS_L1_HINGE = 12,           /* L1HingeLoss (= HingeLoss) */
  SRHIP_LOSS_L2_HINGE = 13,           /* L2HingeLoss */
  SRHIP_LOSS_SMOOTHED_L1_HINGE = 14,  /* SmoothedL1HingeLoss(gamma): p0 = gamma */
  SRHIP_LOSS_MODIFIED_HUBER = 15,     /* ModifiedHuberLoss */
  SRHIP_LOSS_L2_MARGIN = 16,          /* L2MarginLoss */
  SRHIP_LOSS_EXP = 17,                /* ExpLoss */
  SRHIP_LOSS_SIGMOID = 18,            /* SigmoidLoss */
  SRHIP_LOSS_DWD_MARGIN = 19          /* DWDMarginLoss(q): p0 = q */
};

/* One Node{T} (DynamicExpressions v0.16 fields: degree, constant, val, feature, op, l, r;
 * used in the reference at src/Complexity.jl:36-42, src/MutationFunctions.jl:39,52-57).
 * A tree is a contiguous run of nodes; node 0 of the run is the root; l/r index into the run. */
typedef struct srhip_node {
  uint8_t degree;   /* 0 = leaf, 1 = unary, 2 = binary */
  uint8_t constant; /* leaf only: 1 = constant (val), 0 = feature */
  uint16_t op;      /* 1-based index into the binary (degree 2) or unary (degree 1) op list */
  uint16_t feature; /* 1-based feature index (feature leaf) */
  uint16_t pad;
  int32_t l, r;     /* child indices within the tree's node run (-1 = none) */
  double val;       /* constant value; converted to T (exact for F32/I32 values of that type) */
} srhip_node;

typedef struct srhip_operators {
  int32_t nbin, nuna;
  const int32_t* binops; /* [nbin] SRHIP_OP_* code of options.operators.binops[i] */
  const int32_t* unaops; /* [nuna] */
} srhip_operators;

typedef struct srhip_loss {
  int32_t kind; /* SRHIP_LOSS_* */
  int32_t pad;
  double p0, p1;
} srhip_loss;

typedef struct srhip_ctx srhip_ctx;
typedef struct srhip_dataset srhip_dataset;
typedef struct srhip_program srhip_program;

/* thread-local description of the last nonzero status on this thread */
const char* srhip_last_error(void);
/* version string, e.g. "srhip 0.1.0 gfx950" */
const char* srhip_version(void);
/* number of visible HIP devices (0 if none / no driver); never fails */
int srhip_device_count(void);

/* A context owns one device, one stream and device scratch. Not thread-safe: use one
 * context per host thread (e.g. one per Julia task / per island), any number per device. */
int srhip_ctx_create(int device_ordinal, srhip_ctx** out);
void srhip_ctx_destroy(srhip_ctx* ctx);
int srhip_ctx_synchronize(srhip_ctx* ctx);

/* Dataset{T} upload.  Element (feature f, row j) is read from X[f*stride_feature + j*stride_row]
 * (Julia's features x rows column-major matrix: stride_feature = 1, stride_row = nfeatures;
 *  a C/NumPy (nfeatures, n) array: stride_feature = n, stride_row = 1).
 * y may be NULL (prediction-only dataset); weights may be NULL (unweighted).
 * The library copies everything before returning: no host pointer is retained. */
int srhip_dataset_create(srhip_ctx* ctx, int dtype, const void* X, int64_t nfeatures, int64_t n,
                         int64_t stride_feature, int64_t stride_row, const void* y,
                         const void* weights, srhip_dataset** out);
void srhip_dataset_destroy(srhip_dataset* ds);

/* Compile + upload a batch of trees (the population) for one operator table.  ctx may be NULL:
 * a host-only program (compiled, with its did_succeed metadata) usable by srhip_*_finalize and
 * srhip_program_* queries but not by the evaluation calls. */
int srhip_program_create(srhip_ctx* ctx, int dtype, const srhip_node* nodes,
                         const int64_t* tree_offsets /* [ntrees+1] into nodes */, int32_t ntrees,
                         const srhip_operators* ops, srhip_program** out);
void srhip_program_destroy(srhip_program* prog);
/* Number of constant leaves of each tree (DynamicExpressions count_constants order). */
int srhip_program_num_constants(const srhip_program* prog, int32_t* out_nconst /*[ntrees]*/);
/* Replace constant leaves (depth-first, left-to-right = get_constants order), all trees:
 * consts holds sum(nconst) values, tree-major. Re-folds and re-uploads. */
int srhip_program_set_constants(srhip_program* prog, const double* consts);
/* Read the constants back (same layout), e.g. after srhip_optimize_constants. */
int srhip_program_get_constants(const srhip_program* prog, double* consts);

/* Fused evaluate + loss for every tree of prog on ds (rows = all, or idx[0..nidx) 0-based).
 * out_loss[t] = loss in double (L(Inf) = +Inf when !ok), out_ok[t] = did_succeed. */
int srhip_eval_loss(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                    const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                    double* out_loss, uint8_t* out_ok);

/* srhip_eval_loss with one row subset per tree: tree t is evaluated on rows
 * rows[row_offsets[t] .. row_offsets[t+1]) (0-based, duplicates allowed, sets may differ in length).
 * out_loss[t] / out_ok[t] are exactly (same bits) what srhip_eval_loss returns for tree t alone
 * with idx = that set.  The batching mode's fresh minibatch per score (reference:
 * src/LossFunctions.jl:114-127) for a whole population in ONE launch and one synchronisation: each
 * wavefront gathers its tree's rows from the resident dataset itself.  Sets longer than what a wave
 * can stage (40 KB of the set's feature, y and w columns: 1024 rows for Float32 data with 8 features)
 * are evaluated one by one through srhip_eval_loss inside the same call.  srhip_last_kernel_ms reports
 * the rowsets kernel, srhip_last_work the node-rows over the sets. */
int srhip_eval_loss_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                            const srhip_loss* loss, const int64_t* row_offsets /*[ntrees+1]*/,
                            const int64_t* rows, double* out_loss, uint8_t* out_ok);

/* srhip_eval_loss in two halves, for callers that keep the device busy across populations (the
 * reference scores populations from concurrent tasks: Threads.@spawn per population,
 * src/SearchUtils.jl:121-122, @threads_if in src/SingleIteration.jl:112).  _submit queues the
 * evaluation's launches on the context's stream -- behind any evaluation still in flight there -- and
 * returns a ticket at once; _wait blocks until that evaluation has completed, takes its did_succeed
 * decisions and writes out_loss / out_ok exactly as srhip_eval_loss would (same bits), then frees the
 * ticket.  At most 3 tickets per context may be outstanding; tickets may be waited in any order, on
 * the thread that uses the context.  The program and dataset must outlive the ticket.  A row subset
 * (idx != NULL) is evaluated inside _submit (its gather synchronises the stream). */
typedef struct srhip_eval_ticket srhip_eval_ticket;
int srhip_eval_loss_submit(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                           const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                           srhip_eval_ticket** out_ticket);
int srhip_eval_loss_wait(srhip_eval_ticket* ticket, double* out_loss, uint8_t* out_ok);

/* eval_tree_array for every tree: out_pred is T[ntrees][m] (m = n or nidx), row-contiguous. */
int srhip_eval_predict(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                       const int64_t* idx, int64_t nidx, void* out_pred, uint8_t* out_ok);

/* ---- elementwise losses given as expressions (the reference's loss::Function branches of _loss /
 * _weighted_loss, src/LossFunctions.jl:13-33: any l(prediction, target[, weight])) ---------------------
 * A loss l(prediction, target[, weight]) as one Node tree over an operator table.
 * Feature 1 = prediction, 2 = target, 3 = weight (nargs = 3 only).  Constants are val.
 * dtype: SRHIP_F32 / SRHIP_F64 (SRHIP_I32: SRHIP_ERR_UNSUPPORTED).  No device is needed.
 * Operators mean what they mean in a tree of the population (csrc/srhip_ops.h FOps<T>): ^ is safe_pow
 * (NaN for a negative base with a non-integer exponent, ...), log is safe_log (NaN at x <= 0), sqrt is
 * safe_sqrt, and so on -- not the Julia Base functions, which throw there.  Every value is computed in T.
 * Limits, each SRHIP_ERR_INVALID with a message naming it: at most 64 nodes (counting a shared subtree
 * once per use); a stack need of at most 8 (every leaf takes a slot, the child of greater need is
 * evaluated first, two children of equal need cost one slot more); feature indices in 1..nargs; operator
 * indices inside the table; finite constants (in T). */
typedef struct srhip_loss_expr srhip_loss_expr;
int srhip_loss_expr_create(int dtype, const srhip_node* nodes, int64_t nnodes, const srhip_operators* ops,
                           int32_t nargs, srhip_loss_expr** out);
void srhip_loss_expr_destroy(srhip_loss_expr* e);
/* The per-row values l(pred[i], y[i][, w[i]]) in T, computed on the host with the operator bodies of
 * csrc/srhip_ops.h.  w may be NULL for nargs = 2.  No device is needed. */
int srhip_loss_expr_eval_host(const srhip_loss_expr* e, const void* pred, const void* y, const void* w,
                              int64_t n, void* out);
/* srhip_eval_loss with the loss given as an expression: the evaluation of srhip_eval_predict with the
 * predictions left on the device, then one loss pass over them for the trees that succeeded.
 * out_ok[t] = did_succeed of the evaluation, srhip_eval_predict's decision.
 * out_loss[t] = +Inf where !ok, else sum_i l_i / m (unweighted dataset) or sum_i l_i / sum_i w_i (weighted),
 * every l_i in T, the sums in double.  A non-finite l_i is no failure: it propagates into out_loss[t] (NaN
 * or +-Inf) with out_ok[t] = 1, as a Julia closure's would.  out_loss[t] depends on tree t's predictions,
 * the rows and the expression only (fixed summation order: blocks of srhip_lossx_block_rows() rows): the
 * same bits alone or among others, at any position, beside failed trees.
 * A weighted dataset needs nargs = 3, an unweighted one nargs = 2, program and expression the same dtype
 * (SRHIP_ERR_INVALID); an Int32 program is SRHIP_ERR_UNSUPPORTED.  The predictions of the whole program
 * stay resident: ntrees * m * sizeof(T) bytes above SRHIP_LOSSX_MAX_BYTES (environment, read per call,
 * default 8 GiB) is SRHIP_ERR_NOMEM -- split the population.  srhip_last_kernel_ms reports the loss pass
 * (< 0 when no tree succeeded: no loss launch), srhip_last_work what the prediction launch counted. */
int srhip_eval_loss_expr(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                         const srhip_loss_expr* e, const int64_t* idx, int64_t nidx,
                         double* out_loss, uint8_t* out_ok);
/* Rows of one block of the loss pass's summation (a compile-time constant of the library). */
int32_t srhip_lossx_block_rows(void);
/* The compiled program of a loss expression in execution order, for tests.  No device is needed.  *count
 * receives the number of instructions, *need (may be NULL) the value slots the program uses; each of op, dst,
 * a, b, imm (any may be NULL) the first min(count, cap) instructions' fields: op is an operator's device code
 * (srhip_operators) or 0x100 + 0 / 1 / 2 / 3 for a load of the prediction / the target / the weight / a
 * constant; dst the slot written; a and b the slots read (b of a unary operator and a, b of a load are 0); imm
 * a constant load's bits in the expression's type (Float32 in the low word).  The result is in slot 0. */
int srhip_loss_expr_instructions(const srhip_loss_expr* e, uint32_t* op, int32_t* dst, int32_t* a, int32_t* b,
                                 uint64_t* imm, int32_t cap, int32_t* count, int32_t* need);
/* srhip_eval_loss_expr in ONE launch: the interpreter's prediction mode with the loss program
 * behind it in the same kernel, the predictions in a scratch bounded by the launch geometry
 * (srhip_plan_eval_lossx), never ntrees * m.  out_loss / out_ok have exactly the bits of srhip_eval_loss_expr
 * (the same summation order, the same did_succeed decision); argument errors are its own.  There is no
 * residency cap: SRHIP_LOSSX_MAX_BYTES is not read.  srhip_last_kernel_ms reports the fused launch and its
 * finishing sum, srhip_last_work what the launch counted (no tree exits early in prediction mode). */
int srhip_eval_loss_expr_fused(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                               const srhip_loss_expr* e, const int64_t* idx, int64_t nidx,
                               double* out_loss, uint8_t* out_ok);
/* srhip_eval_loss_submit under a loss expression: the fused launch queued on the context's stream, completed
 * by srhip_eval_loss_wait with the bits of srhip_eval_loss_expr.  The ticket is the same type and counts with
 * the built-in tickets towards the 3 a context may have outstanding; any wait order.  A row subset is
 * evaluated inside the call.  Program, dataset and expression must outlive the ticket. */
int srhip_eval_loss_expr_submit(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                                const srhip_loss_expr* e, const int64_t* idx, int64_t nidx,
                                srhip_eval_ticket** out_ticket);
/* The fused launch's geometry, for tests, from shapes and device limits alone.  No device is
 * needed.  rb_rows: rows of an item's row block, a multiple of srhip_lossx_block_rows(); xlds: the block's
 * feature columns are staged in LDS (lds_cols bytes of them fit lds_budget), else read from global memory;
 * tpg trees per item, ngroups tree groups, nblocks row blocks; wgs workgroups, at most wg_per_cu per CU (the
 * workgroups resident at the kernel's register need: 1) and one per item; scratch_bytes = wgs * tpg * rb_rows * sizeof(T): the predictions' scratch.  Returns 0, or a
 * negative value for arguments out of range (null pointers, nlive < 0, m <= 0, maxfeat < 0, num_cu <= 0,
 * lds_max <= 0, a dtype other than SRHIP_F32 / SRHIP_F64). */
typedef struct srhip_lossx_plan_query {
  int32_t dtype;
  int32_t nlive;   /* trees not failed statically */
  int32_t maxfeat; /* staged feature columns */
  int32_t num_cu;
  int64_t m;       /* rows */
  int64_t lds_max; /* the device's LDS bytes per workgroup */
} srhip_lossx_plan_query;
typedef struct srhip_lossx_plan_info {
  int32_t rb_rows, R, xlds, tpg, ngroups, wgs, wg_per_cu, pad;
  int64_t nblocks;
  int64_t lds;           /* dynamic LDS bytes of a workgroup */
  int64_t lds_cols;      /* bytes of the block's feature columns */
  int64_t lds_budget;    /* what a workgroup may stage */
  int64_t scratch_bytes;
} srhip_lossx_plan_info;
int srhip_plan_eval_lossx(const srhip_lossx_plan_query* q, srhip_lossx_plan_info* out);

/* Convenience: program_create + eval_loss + program_destroy. */
int srhip_eval_loss_batch(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_node* nodes,
                          const int64_t* tree_offsets, int32_t ntrees, const srhip_operators* ops,
                          const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                          double* out_loss, uint8_t* out_ok);

/* ---- row-sharded evaluation (several GPUs / processes, each holding a block of rows) -------
 * Replaces nothing in the reference (it has no row parallelism): the reduction
 * of src/LossFunctions.jl:13-33 and the did_succeed checks split into per-shard partials that
 * combine by an all-reduce, then a decision every rank computes identically.
 *   1. srhip_eval_loss_partials on each shard:
 *        sums[2*T + 2*F + 1] (T trees, F features): per tree {sum of (w*)loss, sum of w (or rows)},
 *        per feature {column sum (Float64 data: sum of x * 2^-64), non-finite count}, rows;
 *        chk[T]: operator-output check statistic.
 *   2. all-reduce: sums by SUM; chk by srhip_chk_reduce_op(dtype) (0 = MAX, 1 = SUM).
 *   3. srhip_partials_finalize(prog, F, sums, chk, loss, ok, status): status 2 = undecided
 *      (a near-overflow sum): then 4.
 *   4. srhip_eval_precise_partials for the undecided trees on each shard -> opsums
 *      [n_sel * srhip_program_max_ops(prog)], all-reduce SUM, srhip_precise_finalize -> ok.
 * srhip_eval_loss runs exactly these steps on one device. */
int srhip_eval_loss_partials(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                             const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                             double* sums, double* chk);
int srhip_partials_finalize(const srhip_program* prog, int64_t nfeatures, const double* sums,
                            const double* chk, double* out_loss, uint8_t* out_ok,
                            uint8_t* out_status);
int srhip_eval_precise_partials(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                                const int64_t* idx, int64_t nidx, const int32_t* trees,
                                int32_t ntrees_sel, double* opsums);
int srhip_precise_finalize(const srhip_program* prog, const int32_t* trees, int32_t ntrees_sel,
                           const double* opsums, uint8_t* out_ok);
/* (diagnostic, no device) The decision of tree `tree` evaluated alone on a row set of its own, as
 * srhip_eval_loss_rowsets takes it per tree: rows of the set, feat_stats[3 f ..] = {column sum (Float64
 * data: sum of x * 2^-64), non-finite count (> 0: some), max |x| over the finite entries} of feature f over
 * the set, chk_raw the interpreter's check statistic.  *out_status: 0 ok, 1 fail, 2 undecided; *out_chk
 * (nullable): the statistic decided on (Float32: raised to the tree's +/- bound over the set's features). */
int srhip_decide_rowset(const srhip_program* prog, int32_t tree, int64_t nfeatures, int64_t rows,
                        const double* feat_stats, double chk_raw, uint8_t* out_status, double* out_chk);
int srhip_chk_reduce_op(int dtype);
int32_t srhip_program_max_ops(const srhip_program* prog);

/* ---- multi-GPU exchanges on RCCL (csrc/srhip_comm.cpp; one process per GPU) ------------------
 * Replace the reference's head-node copies between worker processes (Distributed over TCP,
 * src/SearchUtils.jl:108-127): migration (src/Migration.jl:16-38, applied at
 * src/SymbolicRegression.jl:933-943) becomes one all-gather of hall-of-fame / best_sub_pop node
 * tables over xGMI, and row shards combine their partials with one all-reduce.
 * Setup: rank 0 calls srhip_comm_unique_id and broadcasts the SRHIP_COMM_ID_BYTES bytes with the
 * job's launcher; every rank then calls srhip_comm_create with its context (collective: all ranks
 * must call it concurrently).  A communicator owns a HIP stream on its context's device; one
 * exchange at a time (srhip_comm_migrate_start ... srhip_comm_migrate_wait). */
typedef struct srhip_comm srhip_comm;
enum { SRHIP_COMM_ID_BYTES = 128 };
enum { SRHIP_REDUCE_SUM = 0, SRHIP_REDUCE_MAX = 1 };
int srhip_comm_unique_id(uint8_t* out_id /* [SRHIP_COMM_ID_BYTES] */);
int srhip_comm_create(srhip_ctx* ctx, const uint8_t* id, int32_t nranks, int32_t rank, srhip_comm** out);
void srhip_comm_destroy(srhip_comm* comm);
int srhip_comm_size(const srhip_comm* comm, int32_t* nranks, int32_t* rank);
/* Host wall time of the communicator's exchanges (issue -> completion seen; a migration counts from
 * srhip_comm_migrate_start to its _wait): the last one, the total, and how many (any may be NULL). */
int srhip_comm_stats(const srhip_comm* comm, double* ms_last, double* ms_total, int64_t* calls);
/* In-place all-reduce of a float64 vector: on device memory in place, no host staging; a host vector is
 * staged through the communicator's device buffer.  Device memory: the collective runs on the
 * communicator's own stream and is NOT ordered after other streams, so whatever produced buf must be
 * complete when this is called (synchronise the producing stream or event first); the call returns
 * after the collective has completed.  Every exchange waits at most SRHIP_COMM_TIMEOUT_S seconds
 * (default 300) -- past that, or on an asynchronous RCCL error, the communicator is aborted and this
 * and every later call on it fail. */
int srhip_comm_allreduce_f64(srhip_comm* comm, double* buf, int64_t n, int32_t op);
/* Fixed-size all-gather: recv[r * bytes .. (r + 1) * bytes) = rank r's send.  Both device pointers: no
 * staging, and (as for srhip_comm_allreduce_f64) send must be complete before the call; otherwise both
 * are staged through pinned host memory. */
int srhip_comm_allgather(srhip_comm* comm, const void* send, int64_t bytes, void* recv);
/* Migration: this rank's k best trees of (nodes, offsets[ntrees+1], losses[ntrees]) -- by loss,
 * non-finite last, ties by index; trees longer than max_nodes skipped -- packed into one fixed-size
 * payload and all-gathered (issued on the communicator's stream; returns at once).  _wait collects it:
 * out_counts[nranks] trees per rank, out_offsets[nranks][k+1] node offsets within each rank's
 * out_nodes[nranks][k * max_nodes] records, out_losses[nranks][k] (any output may be NULL). */
int srhip_comm_migrate_start(srhip_comm* comm, const srhip_node* nodes, const int64_t* offsets,
                             int32_t ntrees, const double* losses, int32_t k, int32_t max_nodes);
int srhip_comm_migrate_wait(srhip_comm* comm, int32_t* out_counts, int64_t* out_offsets,
                            double* out_losses, srhip_node* out_nodes);
/* Row-sharded eval_loss: ds holds THIS rank's rows (every rank the same features); runs steps 1-4
 * above with the all-reduces on RCCL -- the per-tree partials are written by the reduction straight
 * into the communicator's device buffer and all-reduced there (one group: loss sums, check statistics,
 * the shard's weight / feature / row totals), then copied to the host once; out_loss / out_ok
 * identical on every rank.  With one rank it equals srhip_eval_loss bit for bit. */
int srhip_eval_loss_sharded(srhip_ctx* ctx, srhip_comm* comm, const srhip_dataset* ds,
                            const srhip_program* prog, const srhip_loss* loss, const int64_t* idx,
                            int64_t nidx, double* out_loss, uint8_t* out_ok);

/* ---- constant optimisation (src/ConstantOptimization.jl) ------------------------------------ */
/* Loss and its exact gradient with respect to every tree's constants (forward-mode dual numbers
 * on the device), for every tree of prog: out_loss[T] (+Inf where did_succeed fails; as eval_loss,
 * also +Inf for a succeeding tree whose loss overflows), out_grad[sum nconst] in get_constants order
 * per tree (srhip_program_num_constants), out_ok[T] = did_succeed (srhip_eval_loss's decision).
 * Replaces the finite-difference gradient Optim derives from f(t) = eval_loss(t, dataset,
 * options; regularization=false) (src/ConstantOptimization.jl:48-50); the counterpart of
 * eval_grad_tree_array(tree, X, options; variable=false) (src/InterfaceDynamicExpressions.jl:118-124)
 * reduced through the loss. */
int srhip_eval_loss_grad(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                         const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                         double* out_loss, double* out_grad, uint8_t* out_ok);

/* Per-row derivatives: eval_grad_tree_array(tree, X, options; variable) and eval_diff_tree_array(tree, X,
 * options, direction) (src/InterfaceDynamicExpressions.jl:90-95,118-124; DynamicExpressions v0.16,
 * external) for every tree of prog, forward-mode dual numbers on the device.
 *   wrt = SRHIP_WRT_CONSTANTS: d out / d c for each constant (get_constants order), nconst_t rows per tree
 *   wrt = SRHIP_WRT_FEATURES, direction = 0: d out / d x_f for every feature, nfeatures rows per tree
 *   wrt = SRHIP_WRT_FEATURES, direction = d >= 1: d out / d x_d only, 1 row per tree
 * out_pred: T[ntrees][m] (the evaluator's predictions, as srhip_eval_predict); out_grad: T[sum of rows][m],
 * tree-major, m = n or nidx; out_ok[t] = did_succeed of the evaluation && every derivative finite. */
enum { SRHIP_WRT_CONSTANTS = 0, SRHIP_WRT_FEATURES = 1 };
int srhip_eval_grad_predict(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog, int32_t wrt,
                            int32_t direction, const int64_t* idx, int64_t nidx, void* out_pred, void* out_grad,
                            uint8_t* out_ok);

typedef struct srhip_optim_options {
  int32_t iterations;  /* BFGS iterations per start (Optim.Options(iterations=8), src/Options.jl:693) */
  int32_t nrestarts;   /* perturbed restarts c * (1 + randn/2) (optimizer_nrestarts=2, src/Options.jl:432) */
  uint64_t seed;       /* RNG seed of the restart perturbations */
  double g_tol;        /* gradient infinity-norm tolerance (Optim default 1e-8; <= 0 -> 1e-8) */
} srhip_optim_options;

/* optimize_constants for every tree of prog at once (src/ConstantOptimization.jl:11-81): per tree
 * Newton (one constant) or BFGS (several), each with the BackTracking line search, from the current
 * constants and nrestarts perturbed starts; a tree's constants are replaced (in prog) only where the
 * best minimum beats its baseline loss.  out_loss[T]: the loss of the returned trees (eval_loss,
 * regularization=false); out_improved[T]; out_fcalls[T] (nullable): the reference's num_evals per
 * tree -- objective calls of all starts (result.f_calls) + 1 if improved (the re-score), 0 for a tree
 * without constants or with a static did_succeed failure (left unchanged). */
int srhip_optimize_constants(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                             const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                             const srhip_optim_options* opt, double* out_loss,
                             uint8_t* out_improved, int64_t* out_fcalls);
/* The same, with the restarts' starting points exchanged with the caller
 * (src/ConstantOptimization.jl:53-68: tmptree = copy(tree); val *= T(1) + T(1//2) * randn(T)):
 *   starts_in  (nullable): [nrestarts][sum nconst] restart points in get_constants order, tree-major,
 *              used instead of the library's own draws (a Float32 program rounds them to Float32);
 *   starts_out (nullable): [nrestarts][sum nconst] the restart points actually used.
 * The library's own draws perturb in the program's type: Float32 programs draw a Float32 normal
 * and compute val * (1f + 0.5f * r) in Float32.  Start 0 is always the tree's current constants;
 * its result is kept unless a restart's minimum is strictly smaller (:65-67), and the kept result
 * replaces the constants only if it beats the baseline (:70-78).  Trees without constants or
 * failing statically report their current constants. */
int srhip_optimize_constants_starts(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                    const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                                    const srhip_optim_options* opt, const double* starts_in,
                                    double* starts_out, double* out_loss, uint8_t* out_improved,
                                    int64_t* out_fcalls);

/* ---- row-sharded constant gradients and constant optimisation --------------------------
 * ds holds THIS rank's rows (every rank the same features); every rank calls with the same program, loss,
 * options, seed, starts_in and SRHIP_* environment.  idx indexes the rank's own rows; idx, nidx and the row
 * count may differ between ranks.  A call opens with one exchange of the shards' totals (weight sum or rows,
 * feature statistics, rows) and of the call's signature; if the ranks disagree on a field of it (trees, total
 * constants, dtype, weights, loss kind and parameters, iterations, restarts, seed, g_tol, a hash of starts_in,
 * the SRHIP_OPTIM_* knobs, a forced SRHIP_GRAD_KT) every rank returns SRHIP_ERR_INVALID naming the field.  Every
 * evaluation after it is one exchange: the gradient kernels' shard reduction writes [loss and gradient sums |
 * check statistics] into the communicator's device buffer, the communicator's stream waits for it through an
 * event (no host wait), one RCCL group of at most two all-reduces (SUM; MAX for Float32 statistics), one copy to
 * the host, one host wait.  Every rank takes the same decisions from the same reduced values.
 *   srhip_eval_loss_grad_sharded: srhip_eval_loss_grad's outputs over all ranks' rows, identical on every
 *     rank; with one rank it equals srhip_eval_loss_grad bit for bit.
 *   srhip_optimize_constants_sharded: the contract of srhip_optimize_constants_starts on the objective over all
 *     ranks' rows (baseline and re-score by srhip_eval_loss_sharded); every rank ends with the same constants in
 *     prog.  One group on the caller's context and thread (SRHIP_OPTIM_SPLIT does not apply: a communicator
 *     carries one exchange at a time); SRHIP_GRAD_SCREEN is ignored.  With one rank it equals
 *     srhip_optimize_constants_starts bit for bit.
 * Int32 programs: SRHIP_ERR_UNSUPPORTED.  A communicator with a migration in flight or on another device:
 * SRHIP_ERR_INVALID.  Out of scope: loss expressions (there is no sharded expression scoring to re-score with),
 * row sets, and a rank that fails locally in mid-call -- the others wait out SRHIP_COMM_TIMEOUT_S, as in
 * srhip_eval_loss_sharded. */
int srhip_eval_loss_grad_sharded(srhip_ctx* ctx, srhip_comm* comm, const srhip_dataset* ds, srhip_program* prog,
                                 const srhip_loss* loss, const int64_t* idx, int64_t nidx, double* out_loss,
                                 double* out_grad, uint8_t* out_ok);
int srhip_optimize_constants_sharded(srhip_ctx* ctx, srhip_comm* comm, const srhip_dataset* ds,
                                     srhip_program* prog, const srhip_loss* loss, const int64_t* idx,
                                     int64_t nidx, const srhip_optim_options* opt, const double* starts_in,
                                     double* starts_out, double* out_loss, uint8_t* out_improved,
                                     int64_t* out_fcalls);
/* The manual steps, beside srhip_eval_loss_partials, for shards combined by any transport:
 *   1. srhip_eval_loss_grad_partials on each shard: sums[2*T + 2*F + 1] as srhip_eval_loss_partials lays them
 *      out (the loss sums are the gradient kernels'), gsums[sum nconst] the gradient sums in get_constants
 *      order, chk[T] the gradient program's check statistic (Float32: a non-finite one is +Inf).
 *   2. combine: sums and gsums by SUM, chk by srhip_chk_reduce_op(dtype).
 *   3. srhip_grad_partials_finalize (no device): out_loss[T] and out_grad[sum nconst] over the combined weight
 *      sum, out_ok[T], out_status[T] (nullable); a failing tree is +Inf with a zero slice; status 2 =
 *      undecided: then step 4 of the evaluation (srhip_eval_precise_partials, SUM, srhip_precise_finalize),
 *      and a tree that fails there becomes +Inf with a zero slice.  prog is the program step 1 ran on, at the
 *      same constants, or a host-only program (ctx = NULL) of the same trees.
 * srhip_shard_signature_check (no device): reduced[2 * nfields] holds the MAX over the ranks of [k_i, -k_i] per
 * field; returns the first field with max(k_i) != -max(-k_i), or -1 (-2: a null argument).  The library's own
 * signature has srhip_shard_signature_fields() fields, named by srhip_shard_signature_field_name. */
int srhip_eval_loss_grad_partials(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                  const srhip_loss* loss, const int64_t* idx, int64_t nidx, double* sums,
                                  double* gsums, double* chk);
int srhip_grad_partials_finalize(srhip_program* prog, int64_t nfeatures, const double* sums,
                                 const double* gsums, const double* chk, double* out_loss, double* out_grad,
                                 uint8_t* out_ok, uint8_t* out_status);
int32_t srhip_shard_signature_check(const double* reduced, int32_t nfields);
int32_t srhip_shard_signature_fields(void);
const char* srhip_shard_signature_field_name(int32_t field);

/* srhip_eval_loss_grad with the loss given as an expression (srhip_loss_expr): the same dual-number launch
 * over (tree, constant chunk) pairs, its loss stage running the expression's program over dual numbers with
 * one tangent, d / d prediction (every operator's value and partials are the ones the trees' own operators
 * use).  out_ok[t] is srhip_eval_loss_grad's decision for the tree -- the expression's outputs take no part
 * in it.  Where it is 0: out_loss[t] = +Inf and the tree's gradient slice is 0.  Elsewhere out_loss[t] =
 * sum_i l_i / m (unweighted dataset) or / sum_i w_i (weighted; the expression names the weight itself, the
 * kernel does not multiply by it), and the slice is sum_i dl_i * d pred_i / d c_k over the same denominator,
 * every l_i, dl_i and product in T, the sums in double in the fixed order of srhip_eval_loss_grad (the same
 * bits alone or among others).  A non-finite result is passed through with ok = 1.  For square(p - t) and
 * w * square(p - t) the results have the bits of srhip_eval_loss_grad under SRHIP_LOSS_L2.
 * Argument errors as srhip_eval_loss_expr; srhip_last_kernel_ms reports the gradient kernels. */
int srhip_eval_loss_grad_expr(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                              const srhip_loss_expr* e, const int64_t* idx, int64_t nidx,
                              double* out_loss, double* out_grad, uint8_t* out_ok);
/* srhip_optimize_constants_starts under a loss expression.  Baseline and final re-score are
 * srhip_eval_loss_expr's (out_loss[t] has its bits on the returned constants); the objective is
 * srhip_eval_loss_grad_expr's kernel.  Inside the optimiser an objective value that is not finite (NaN or
 * +-Inf) counts as +Inf before the line search or the acceptance test sees it (LineSearches' BackTracking
 * shrinks on !isfinite); everything else -- methods, restarts, starts_in / starts_out, acceptance,
 * out_fcalls -- is srhip_optimize_constants_starts.  Argument errors as srhip_eval_loss_expr; a failed
 * call leaves prog's constants unchanged. */
int srhip_optimize_constants_expr(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                  const srhip_loss_expr* e, const int64_t* idx, int64_t nidx,
                                  const srhip_optim_options* opt, const double* starts_in,
                                  double* starts_out, double* out_loss, uint8_t* out_improved,
                                  int64_t* out_fcalls);

/* srhip_eval_loss_grad with one row subset per tree (row_offsets / rows as srhip_eval_loss_rowsets:
 * 0-based rows, duplicates allowed, sets may differ in length; empty sets, non-monotone offsets,
 * out-of-range rows and null pointers are SRHIP_ERR_INVALID naming the tree and the position; Int32
 * programs are SRHIP_ERR_UNSUPPORTED).  out_loss[t], tree t's slice of out_grad and out_ok[t] are exactly
 * (same bits) what srhip_eval_loss_grad returns for tree t alone, in a one-tree program, with idx = its
 * set.  The objective of the batching mode's optimize_constants, where every member has a minibatch of
 * its own (src/ConstantOptimization.jl:14-17 batch_sample per member, :48 its idx in f), for a whole
 * population in one launch: the sets are gathered once into a packed device buffer, one wavefront per
 * (tree, constant chunk) copies its set into LDS and walks it in the 256-row blocks of the single-idx
 * kernel, combining the block records in that path's reduction order.  The derived view of the
 * single-idx path is off below 8192 rows, so it never applies to a staged set.  Sets longer than a wave
 * can stage (40 KB of the set's feature, y and w columns, in whole 256-row blocks: 1536 rows for Float32
 * data with 5 features, 768 for Float64) go through srhip_eval_loss_grad one by one inside the same
 * call.  srhip_last_kernel_ms reports the row-set gradient kernel. */
int srhip_eval_loss_grad_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                 const srhip_loss* loss, const int64_t* row_offsets /*[ntrees+1]*/,
                                 const int64_t* rows, double* out_loss, double* out_grad,
                                 uint8_t* out_ok);

/* srhip_optimize_constants_starts with one row subset per tree: optimize_constants in batching mode
 * (src/ConstantOptimization.jl:11-81, where :14-17 draws batch_sample(dataset, options) per member and
 * the member's BFGS / Newton run, its restarts and its re-score all use that idx, :48, :72) for a whole
 * population in one call, one launch per optimiser round over every tree still active.  For every tree,
 * out_loss[t], out_improved[t], out_fcalls[t], the constants left in prog and its slice of starts_out
 * are exactly (same bits) what srhip_optimize_constants_starts returns for tree t alone, with idx = its
 * set and opt->seed = tree_seeds[t].
 *   tree_seeds (nullable): [ntrees] the seed of tree t's own generator (NULL: opt->seed + t); its restart
 *              points are drawn from that generator and a fresh normal distribution, start-major and then
 *              constant by constant -- the sequence of the one-tree call;
 *   starts_in / starts_out (nullable): the layout of srhip_optimize_constants_starts
 *              ([nrestarts][sum nconst]); starts_in replaces the draws.
 * Baseline and final re-score are one srhip_eval_loss_rowsets launch each; acceptance and out_fcalls
 * follow srhip_optimize_constants.  Row-set conventions, validation and the handling of sets no wave
 * can stage (the single-idx optimiser on that tree, inside the call) as srhip_eval_loss_grad_rowsets;
 * a failed call leaves prog's constants unchanged. */
int srhip_optimize_constants_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                     const srhip_loss* loss, const int64_t* row_offsets /*[ntrees+1]*/,
                                     const int64_t* rows, const srhip_optim_options* opt,
                                     const uint64_t* tree_seeds /*[ntrees], nullable*/,
                                     const double* starts_in /*nullable*/, double* starts_out /*nullable*/,
                                     double* out_loss, uint8_t* out_improved, int64_t* out_fcalls);

/* ---- loss expressions with one row subset per tree (batching mode under a custom elementwise_loss) ----
 * row_offsets / rows, their validation (SRHIP_ERR_INVALID naming tree and position) and the meaning of
 * "alone, in a one-tree program, with idx = its set" are those of srhip_eval_loss_rowsets; the expression's
 * argument errors are srhip_eval_loss_expr's (nargs against the weighted / unweighted dataset, dtype,
 * SRHIP_ERR_UNSUPPORTED for an Int32 program).  Two kinds of tree are settled inside the call by the one-tree
 * single-idx expression call itself: a set longer than the entry point's cap, and (scoring) a tree whose
 * record leaves the did_succeed decision open (near overflow).  srhip_rowsets_fallback_trees counts them.
 *
 * srhip_eval_loss_expr_rowsets: out_loss[t] / out_ok[t] are exactly (same bits) srhip_eval_loss_expr's.  One
 * launch and one synchronisation: each wavefront stages its tree's rows by index, runs the interpreter in its
 * prediction mode, then the loss program over its predictions, summing in the loss pass's order (blocks of
 * srhip_lossx_block_rows() rows).  Cap: srhip_eval_loss_rowsets' (40 KB of the set's feature, y and w
 * columns in whole tiles -- the predictions live in device scratch: 5120 rows for Float32 data with one
 * feature, 1024 with 8 features and weights). */
int srhip_eval_loss_expr_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog,
                                 const srhip_loss_expr* e, const int64_t* row_offsets /*[ntrees+1]*/,
                                 const int64_t* rows, double* out_loss, uint8_t* out_ok);
/* out_loss[t], tree t's slice of out_grad and out_ok[t] are exactly (same bits) srhip_eval_loss_grad_expr's.
 * The launch is srhip_eval_loss_grad_rowsets' (packed sets, one wavefront per (tree, constant chunk), 256-row
 * blocks) with the expression's dual program as its loss stage.  Cap: srhip_eval_loss_grad_rowsets' (whole
 * 256-row blocks under the same 40 KB: 1536 rows for Float32 data with 5 features, 768 for Float64). */
int srhip_eval_loss_grad_expr_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                      const srhip_loss_expr* e, const int64_t* row_offsets /*[ntrees+1]*/,
                                      const int64_t* rows, double* out_loss, double* out_grad,
                                      uint8_t* out_ok);
/* For every tree, out_loss[t], out_improved[t], out_fcalls[t], the constants left in prog and its slice of
 * starts_out are exactly (same bits) what srhip_optimize_constants_expr returns for tree t alone, with idx =
 * its set and opt->seed = tree_seeds[t] (NULL: opt->seed + t).  Baseline and final re-score are one
 * srhip_eval_loss_expr_rowsets launch each; an objective value that is not finite counts as +Inf
 * (srhip_optimize_constants_expr's rule); restart draws, starts_in / starts_out, acceptance and out_fcalls as
 * srhip_optimize_constants_rowsets.  Cap: srhip_eval_loss_grad_expr_rowsets' (a longer set: the single-idx
 * optimiser on that tree, inside the call).  A failed call leaves prog's constants unchanged. */
int srhip_optimize_constants_expr_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* prog,
                                          const srhip_loss_expr* e, const int64_t* row_offsets /*[ntrees+1]*/,
                                          const int64_t* rows, const srhip_optim_options* opt,
                                          const uint64_t* tree_seeds /*[ntrees], nullable*/,
                                          const double* starts_in /*nullable*/, double* starts_out /*nullable*/,
                                          double* out_loss, uint8_t* out_improved, int64_t* out_fcalls);

/* ---- measurement hooks (bench / profiling) --------------------------------------------- */
/* Device time (ms) of the last main kernel on this context -- the interpreter of srhip_eval_loss /
 * srhip_eval_predict, or the dual-number kernel of srhip_eval_loss_grad -- measured with HIP events
 * recorded on the context's stream; < 0 if unavailable (also after srhip_optimize_constants*, whose
 * many small gradient launches go without events). */
double srhip_last_kernel_ms(const srhip_ctx* ctx);
/* Work of the last srhip_eval_loss / srhip_eval_loss_partials / srhip_eval_predict on this context,
 * counted on the device (the rows each tree was actually evaluated on: a tree that failed -- the
 * reference's early return -- stops at the failing tile): out[0] evaluated node-rows (count_nodes x
 * rows), out[1] nominal node-rows (every live tree on every row), out[2] evaluated operator-node
 * rows, out[3] evaluated tree-rows. */
int srhip_last_work(const srhip_ctx* ctx, int64_t out[4]);
/* Launches of the interpreter's hot form on this context so far (the persistent main
 * launch of the wide Float32 loss kernel with its per-slot records); < 0 for a null context.  The
 * tests' way to see which form evaluated a population. */
int64_t srhip_hot_form_launches(const srhip_ctx* ctx);
/* Trees of the last row-set call on this context (srhip_eval_loss*_rowsets, srhip_eval_loss_grad*_rowsets,
 * srhip_optimize_constants*_rowsets) that were settled by the one-tree single-idx call instead of the
 * row-set kernel: sets over the cap and, when scoring, undecided trees; < 0 for a null context.  The tests'
 * way to tell the kernel from the fallback. */
int64_t srhip_rowsets_fallback_trees(const srhip_ctx* ctx);
/* Per-program work counters: sum over trees of count_nodes / operator nodes. */
int srhip_program_stats(const srhip_program* prog, int64_t* total_nodes, int64_t* total_opnodes,
                        int32_t* max_stack);
/* Derived columns of a program (heavy unary operators on feature leaves computed once per
 * workgroup and shared by every tree): count, and if spec is non-null the first
 * min(count, cap) entries as (device unary op << 16) | (feature - 1).  Set SRHIP_NO_DERIVE=1
 * before srhip_program_create to compile without them. */
int srhip_program_derived(const srhip_program* prog, int32_t* count, uint32_t* spec, int32_t cap);
/* The interpreter's instruction set, for tests and diagnostics (no device is needed).  Handler ids run
 * from 0 to srhip_isa_handler_count() - 1; srhip_isa_handler_name writes an id's name ("END", "LOADF",
 * "PUSHLC2", "SUB.SA3", "ADD.FC", "POW.AS0", "UN.erfc": operator, operand form, stack slot) into buf;
 * srhip_isa_handler_ok returns 1 if the kernels of element type dtype implement the handler, 0 if not
 * (Int32 has the ring operators and comparisons only), a negative value for arguments out of range. */
int32_t srhip_isa_handler_count(void);
int srhip_isa_handler_name(uint32_t h, char* buf, int32_t cap);
int srhip_isa_handler_ok(uint32_t h, int dtype);
/* The handler ids of one tree's evaluation program in execution order, its END included, as a launch
 * runs them: after constant folding and the superinstruction pass, through the code cache.  derived
 * != 0: the derived-column program (srhip_program_derived) when the program has one, which launches
 * prefer; 0: the plain program.  *count receives the length; out (may be NULL) the first min(count,
 * cap) ids.  A tree the host already decided as failed is its END alone. */
int srhip_program_handlers(const srhip_program* prog, int32_t tree, int32_t derived, uint32_t* out, int32_t cap,
                           int32_t* count);
/* Process-wide counters of the per-tree code cache used by srhip_program_create (any argument may be
 * NULL): trees served from the cache, trees compiled, entries made (a tree gets an entry on its
 * second sighting; SRHIP_CODE_CACHE_EAGER=1: on its first). */
int srhip_code_cache_stats(int64_t* hits, int64_t* misses, int64_t* inserts);
/* The persistent launch's last-round plan, for tests: the parts of share `share` when
 * `blocks` leftover row blocks of `units` units each are dealt to `nshares` >= blocks shares.  Writes
 * up to two parts as (block, first unit, end unit) triples to out[6] and returns their number (0: an
 * empty share), or a negative value for arguments out of range.  No device is needed. */
int srhip_tail_share_parts(int32_t blocks, int32_t units, int32_t nshares, int32_t share, int32_t* out);
/* How an evaluation would run (the launch plan), for tests: the decision eval launches
 * and the order pre-planned at srhip_program_create both take, from shapes, device limits and the
 * SRHIP_* switches of the calling process.  No device is needed.  kind: 0 small-population, 1
 * persistent, 2 grid launch; mode: 0 loss, 1 prediction, 2 precise pass.  Returns 0, or a negative
 * value for arguments out of range (null pointers, nlive < 0, m <= 0, num_cu <= 0, lds_max <= 0, an
 * unknown dtype or mode). */
typedef struct srhip_plan_query {
  int32_t dtype, mode;    /* SRHIP_F32 / F64 / I32 */
  int32_t nlive;          /* trees not failed statically */
  int32_t maxfeat, nd;    /* staged feature columns, derived columns */
  int32_t kmax, dkmax;    /* stack depth of the plain / derived-column program */
  int32_t wide_ops;       /* asin, acos or atanh_clip among the unary operators */
  int32_t weighted, sharded, have_recs;
  int32_t loss_kind;
  int32_t num_cu;
  int32_t pad;
  int64_t m;              /* rows */
  int64_t lds_max;        /* the device's LDS bytes per workgroup */
} srhip_plan_query;
typedef struct srhip_plan_info {
  int32_t kind, R, K, use_d;
  int32_t rb_rows, nrb, groups, tpg, xlds;
  int32_t nch, cpb, wg_waves;
  int32_t probe_blocks, probe_tile_claims, wgs;
  int32_t tail_slices, tail_blocks, tail_shares, expect_items;
  int32_t fused, hot;
  int32_t pad;
  int64_t lds;            /* LDS bytes of a workgroup */
} srhip_plan_info;
int srhip_plan_eval(const srhip_plan_query* q, srhip_plan_info* out);
/* The constant optimiser's state machine (srhip_optimize_constants: BFGS / one-constant Newton over
 * BackTracking, best of the starts, value-only trials, speculative trial points) over a callback instead
 * of the device, for tests.  No device is needed.  Every tree t with constants (const_offsets[t + 1] >
 * const_offsets[t]) is optimised from starts[s][const_offsets[t] ..], s = 0 .. nstarts - 1; best_x
 * ([sum nconst]), best_f and fcalls ([ntrees]) receive its best point, that point's objective and its
 * objective calls; entries of trees without constants, and every output of a failed call, stay as they
 * are.  *nlaunches (may be NULL): the callback calls made.  Each call evaluates nitems items: item i is
 * tree tree[i] at the point x[x_off[i] ..] -- a tree's own next point, or a speculative one (at most
 * spec_slots per call).  It writes f[i], finite or +Inf, and, unless value_only[i], the gradient at
 * g[x_off[i] ..]; a non-zero result ends the run and is returned.  g_tol <= 0: 1e-8. */
typedef int (*srhip_bfgs_eval_fn)(void* user, int32_t nitems, const int32_t* tree, const int64_t* x_off,
                                  const double* x, const uint8_t* value_only, double* f, double* g);
typedef struct srhip_bfgs_query {
  int32_t ntrees, nstarts;
  const int64_t* const_offsets; /* [ntrees + 1] */
  const double* starts;         /* [nstarts][sum nconst] */
  int32_t iterations;
  int32_t value_trials;         /* trials after a line search's first are value-only */
  int32_t spec_slots, spec_max_active, spec_max_depth; /* SRHIP_OPTIM_SPEC / _SPEC_ACTIVE / _SPEC_DEPTH */
  int32_t pad;
  double g_tol;
} srhip_bfgs_query;
int srhip_bfgs_host(const srhip_bfgs_query* q, srhip_bfgs_eval_fn eval, void* user, double* best_x, double* best_f,
                    int64_t* fcalls, int64_t* nlaunches);

/* ---- Cross-population request coalescer (8(b) "Threading") ----------------
 * The reference scores one tree per mutation from every population task concurrently
 * (score_func in next_generation, src/Mutate.jl:268-274, under Threads.@spawn per population,
 * src/SymbolicRegression.jl:964-987 / src/SearchUtils.jl:121-122).  A batcher uses the caller's
 * context and device dataset; any number of threads submit single-tree score requests and block on
 * their ticket; worker threads (SRHIP_COALESCE_WORKERS, default 2: worker 0 on the caller's context,
 * the others on contexts of their own on the same device, so one compiles and launches while
 * another waits for its kernel) flush the queue as ONE program + ONE srhip_eval_loss launch
 * when max_batch requests are queued, when every registered client is waiting (nclients > 0), or
 * max_wait_us after the oldest request.  Requests with different row subsets (batching `idx`)
 * go to separate launches of the same flush.  Results are exactly those of srhip_eval_loss on
 * the single tree (the kernel's per-tree results do not depend on the batch).  Thread-safe; the
 * context must not be used by other callers while the batcher lives. */
typedef struct srhip_batcher srhip_batcher;
int srhip_batcher_create(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_operators* ops,
                         const srhip_loss* loss, int32_t max_batch, int32_t max_wait_us,
                         srhip_batcher** out);
/* The same coalescer under a loss given as an expression: a flush is one program plus ONE fused launch
 * (srhip_eval_loss_expr_fused), its subset group one srhip_eval_loss_expr_rowsets launch.  A request's result
 * has the bits of srhip_eval_loss_expr on that tree alone.  The dataset must suit the expression (dtype,
 * nargs against its weights: srhip_eval_loss_expr's errors, reported here); the expression must outlive the
 * batcher.  Every other srhip_batcher_* entry is unchanged. */
int srhip_batcher_create_expr(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_operators* ops,
                              const srhip_loss_expr* e, int32_t max_batch, int32_t max_wait_us,
                              srhip_batcher** out);
/* expected number of concurrent clients (0 = unknown: flush on max_batch / max_wait_us only) */
int srhip_batcher_set_clients(srhip_batcher* b, int32_t nclients);
/* one tree (nodes[0] is its root); idx = optional 0-based row subset (copied) */
int srhip_batcher_submit(srhip_batcher* b, const srhip_node* nodes, int64_t nnodes,
                         const int64_t* idx, int64_t nidx, uint64_t* ticket);
/* blocks until the ticket's batch ran; returns that request's status (errors carry the message
 * of the failed compile / launch, readable with srhip_last_error on the waiting thread) */
int srhip_batcher_wait(srhip_batcher* b, uint64_t ticket, double* out_loss, uint8_t* out_ok);
/* submit + wait */
int srhip_batcher_eval(srhip_batcher* b, const srhip_node* nodes, int64_t nnodes,
                       const int64_t* idx, int64_t nidx, double* out_loss, uint8_t* out_ok);
/* requests served, device launches, largest batch */
int srhip_batcher_stats(const srhip_batcher* b, int64_t* nrequests, int64_t* nlaunches,
                        int64_t* max_batch_seen);
/* worker wall time spent inside flushes (compile + upload + launch + wait, ms, summed over the
 * workers) and the summed interpreter-kernel time of their launches (HIP events, ms): kernel_ms /
 * elapsed wall time is the device-busy fraction of a search (bench C1 / C3; concurrent launches of
 * two workers can overlap, so it is an upper bound) */
int srhip_batcher_timing(const srhip_batcher* b, double* busy_ms, double* kernel_ms);
/* drains the queue (pending requests are evaluated), joins the worker */
void srhip_batcher_destroy(srhip_batcher* b);

#ifdef __cplusplus
}
#endif
#endif /* SRHIP_H */
