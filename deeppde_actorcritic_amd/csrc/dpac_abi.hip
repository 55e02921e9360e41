// dpac_abi.hip — the extern "C" surface of libdpac (include/dpac.h): argument
// validation, thread-local error reporting and dispatch to the per-equation
// kernel instantiations and the other TUs' launchers (dpac_host.h).
#include <cstdarg>
#include <cstdio>
#include <string>

#include "dpac_host.h"
#include "dpac_kernels.h"

namespace dpac {
// The instantiation table the equation TUs fill at load time (Registrar, dpac_launch.h):
// [equation id][dim][f64] (dim up to kMaxRegDim, dpac_launch.h, checked at build time by
// Registrar).  Zero-initialised before any constructor runs.
static DispatchFn g_dispatch[4][kMaxRegDim + 1][2];
void register_dispatch(int eqn, int dim, int f64, DispatchFn fn) {
  if (eqn >= 0 && eqn < 4 && dim >= 1 && dim <= kMaxRegDim && (f64 == 0 || f64 == 1)) g_dispatch[eqn][dim][f64] = fn;
}
DispatchFn find_dispatch(int eqn, int dim, int f64) {
  if (eqn < 0 || eqn >= 4 || dim < 1 || dim > kMaxRegDim || (f64 != 0 && f64 != 1)) return nullptr;
  return g_dispatch[eqn][dim][f64];
}

namespace {
thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int ok() {
  g_err.clear();
  return DPAC_OK;
}

// the tail of every entry point that launches outside the dispatch table
int finish(int r) {
  if (r != 0) return fail(r, "kernel launch failed: %s", hipGetErrorString((hipError_t)r));
  return ok();
}

int check_dtype(int32_t dtype) {
  if (dtype != DPAC_F32 && dtype != DPAC_F64) return fail(DPAC_EINVAL, "bad dtype %d", dtype);
  return DPAC_OK;
}

int check_rows(int64_t rows) {
  if (rows < 1) return fail(DPAC_EINVAL, "rows must be >= 1 (got %lld)", (long long)rows);
  return DPAC_OK;
}

int check_cost_order(int32_t cost_order) {
  if (cost_order != DPAC_COST_CRITIC && cost_order != DPAC_COST_ACTOR)
    return fail(DPAC_EINVAL, "bad cost_order %d", cost_order);
  return DPAC_OK;
}

int check_eq(const dpac_eqn_params* eq) {
  if (!eq) return fail(DPAC_EINVAL, "eqn params pointer is NULL");
  if (eq->reserved != 0) return fail(DPAC_EINVAL, "eqn params: reserved must be 0");
  if (eq->dim < 1) return fail(DPAC_EINVAL, "dim must be >= 1 (got %d)", eq->dim);
  switch (eq->eqn) {
    case DPAC_EQN_LQR:
    case DPAC_EQN_EKN:
    case DPAC_EQN_LQR_VAR:
      if (eq->control_dim != eq->dim)
        return fail(DPAC_EINVAL, "control_dim (%d) must equal dim (%d) for this equation",
                    eq->control_dim, eq->dim);
      break;
    case DPAC_EQN_VDP:
      if (eq->dim != 2 * eq->control_dim)
        return fail(DPAC_EINVAL, "VDP needs dim == 2*control_dim (dim %d, control_dim %d)",
                    eq->dim, eq->control_dim);
      break;
    default:
      return fail(DPAC_EINVAL, "unknown equation id %d", eq->eqn);
  }
  if (!(eq->R > 0)) return fail(DPAC_EINVAL, "R must be > 0");
  const bool has = find_dispatch(eq->eqn, eq->dim, 0) && find_dispatch(eq->eqn, eq->dim, 1);
  if (!has)
    return fail(DPAC_EUNSUP, "equation %d has no kernel instantiation for dim %d", eq->eqn,
                eq->dim);
  return DPAC_OK;
}

int check_common(const dpac_eqn_params* eq, int32_t dtype, int64_t B) {
  if (int e = check_eq(eq)) return e;
  if (int e = check_dtype(dtype)) return e;
  if (B < 1) return fail(DPAC_EINVAL, "num_sample must be >= 1 (got %lld)", (long long)B);
  if (B > (int64_t)1 << 31) return fail(DPAC_EINVAL, "num_sample too large");
  return DPAC_OK;
}

// check_common and the time grid of the entry points that step the SDE
int check_run(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype, int64_t B, int32_t N, double T) {
  if (int e = check_common(eq, dtype, B)) return e;
  if (scheme != DPAC_SCHEME_NAIVE && scheme != DPAC_SCHEME_ADAPTIVE)
    return fail(DPAC_EINVAL, "bad scheme %d", scheme);
  if (N < 1) return fail(DPAC_EINVAL, "num_steps must be >= 1 (got %d)", N);
  if (!(T > 0)) return fail(DPAC_EINVAL, "total_time must be > 0");
  return DPAC_OK;
}

int check_sample_type(int32_t st) {
  if (st != DPAC_SAMPLE_NORMAL && st != DPAC_SAMPLE_BOUNDED && st != DPAC_SAMPLE_ZERO_X0)
    return fail(DPAC_EINVAL, "bad sample_type %d", st);
  return DPAC_OK;
}

// the increments of sample0 are the normal ones (only its x0 differs)
int dw_sample_type(int32_t st) { return st == DPAC_SAMPLE_ZERO_X0 ? DPAC_SAMPLE_NORMAL : st; }

// A dpac_mlp for the row-parallel kernels (no equation attached); `who` heads the messages.
int check_net(const dpac_mlp* net, const char* who = "") {
  if (!net) return fail(DPAC_EINVAL, "%sMLP pointer is NULL", who);
  const int L = net->n_hidden;
  if (L < 1 || L > DPAC_MLP_MAX_HIDDEN)
    return fail(DPAC_EINVAL, "%sn_hidden must be in [1, %d] (got %d)", who, DPAC_MLP_MAX_HIDDEN, L);
  for (int i = 0; i <= L + 1; ++i) {
    if (net->width[i] < 1 || net->width[i] > DPAC_MLP_MAX_WIDTH)
      return fail(DPAC_EINVAL, "%swidth[%d] = %d outside [1, %d]", who, i, net->width[i],
                  DPAC_MLP_MAX_WIDTH);
    if (!net->bn_scale[i] || !net->bn_shift[i])
      return fail(DPAC_EINVAL, "%sbn_scale/bn_shift[%d] is NULL", who, i);
  }
  if (!net->bias) return fail(DPAC_EINVAL, "%sbias is NULL", who);
  // guard_phase: one of DPAC_GUARD_*, and a split phase only with a status word
  if (net->guard_phase < DPAC_GUARD_INLINE || net->guard_phase > DPAC_GUARD_FALLBACK_ONLY)
    return fail(DPAC_EINVAL, "%sguard_phase must be 0, 1 or 2 (got %d)", who, net->guard_phase);
  if (net->guard_phase != DPAC_GUARD_INLINE && !net->status)
    return fail(DPAC_EINVAL, "%sguard_phase %d needs a status word", who, net->guard_phase);
  return DPAC_OK;
}

// net->weight[] (the entry points that read the weights; the parameter gradients do not)
int check_weights(const dpac_mlp* net, const char* who = "") {
  for (int i = 0; i <= net->n_hidden; ++i)
    if (!net->weight[i]) return fail(DPAC_EINVAL, "%sweight[%d] is NULL", who, i);
  return DPAC_OK;
}

// the backward entry points' weight_t argument
int check_weight_t(const dpac_mlp* net, const void* const* weight_t) {
  if (!weight_t) return fail(DPAC_EINVAL, "required pointer 'weight_t' is NULL");
  for (int i = 0; i <= net->n_hidden; ++i)
    if (!weight_t[i]) return fail(DPAC_EINVAL, "weight_t[%d] is NULL", i);
  return DPAC_OK;
}

// The net a backward entry point hands on: the struct's weight_km (forward images) never reach
// the backward, which reads the images of weight_t.
dpac_mlp backward_net(const dpac_mlp* net, const void* const* weight_t_km) {
  dpac_mlp b = *net;
  for (int i = 0; i <= net->n_hidden; ++i) b.weight_km[i] = weight_t_km ? weight_t_km[i] : nullptr;
  return b;
}

// The actor of the fused rollout: a net whose ends fit the equation.
int check_mlp(const dpac_eqn_params* eq, const dpac_mlp* actor) {
  if (int e = check_net(actor, "actor: ")) return e;
  if (int e = check_weights(actor, "actor: ")) return e;
  const int L = actor->n_hidden;
  if (actor->ekn_head != 0 && actor->ekn_head != 1)
    return fail(DPAC_EINVAL, "actor: ekn_head must be 0 or 1");
  if (actor->ekn_head && eq->eqn != DPAC_EQN_EKN)
    return fail(DPAC_EINVAL, "actor: the Eikonal head applies to the EKN equation only");
  if (actor->width[0] != eq->dim)
    return fail(DPAC_EINVAL, "actor: width[0] (%d) must equal dim (%d)", actor->width[0], eq->dim);
  if (actor->width[L + 1] != eq->control_dim + actor->ekn_head)
    return fail(DPAC_EINVAL, "actor: output width %d must be control_dim%s (%d)",
                actor->width[L + 1], actor->ekn_head ? " + 1" : "",
                eq->control_dim + actor->ekn_head);
  return DPAC_OK;
}

int check_adam_tensors(int32_t dtype, int32_t n, const int64_t* numel, void* const* var,
                       const void* const* grad, void* const* m, void* const* v) {
  if (int e = check_dtype(dtype)) return e;
  if (n < 0) return fail(DPAC_EINVAL, "n_tensors must be >= 0 (got %d)", n);
  if (n > 0 && (!numel || !var || !grad || !m || !v))
    return fail(DPAC_EINVAL, "numel, var, grad, m and v are required pointers with n_tensors > 0");
  for (int i = 0; i < n; ++i) {
    if (numel[i] < 1) return fail(DPAC_EINVAL, "tensor %d: numel must be >= 1", i);
    if (!var[i] || !grad[i] || !m[i] || !v[i])
      return fail(DPAC_EINVAL, "tensor %d: a pointer is NULL", i);
  }
  return DPAC_OK;
}

#define DPAC_REQUIRE(ptr) \
  if (!(ptr)) return fail(DPAC_EINVAL, "%s: required pointer '%s' is NULL", __func__, #ptr)

OpArgs blank(const dpac_eqn_params* eq, int op, int32_t scheme, int32_t dtype, int64_t B, int32_t N,
             double T, void* stream) {
  OpArgs a{};
  a.op = op;
  a.eq = *eq;
  a.scheme = scheme; a.dtype = dtype; a.B = B; a.N = N; a.T = T;
  a.stream = (hipStream_t)stream;
  return a;
}

// the dispatch-table call every launch ends in, after its size checks
int dispatch(const OpArgs& a) {
  const DispatchFn fn = find_dispatch(a.eq.eqn, a.eq.dim, a.dtype == DPAC_F64 ? 1 : 0);
  const int r = fn ? fn(a) : DPAC_EUNSUP;
  if (r == DPAC_EUNSUP) return fail(r, "no kernel for equation %d dim %d", a.eq.eqn, a.eq.dim);
  return finish(r);
}

int launch(const OpArgs& a) {
  const bool f64 = a.dtype == DPAC_F64;
  // Kernels address each [N+1][B][d] / [N][B][c] / [B][N] array through one
  // 32-bit buffer descriptor whose offsets >= 2^31 mean "out of range".
  const int64_t esz = f64 ? 8 : 4;
  const int64_t width = a.eq.dim > a.eq.control_dim ? a.eq.dim : a.eq.control_dim;
  // B <= 2^31 and width <= 2^31 are checked before, so row_bytes cannot overflow; the step
  // count is compared by division (B * width * (N + 1) * esz overflows int64 for huge N:
  // found by the host UBSan run, tests/abi_sanitize.c)
  if (width > (1 << 16)) return fail(DPAC_EINVAL, "dim %d / control_dim %d too large", a.eq.dim, a.eq.control_dim);
  const int64_t limit = (int64_t)1 << 31, row_bytes = a.B * width * esz;
  if (row_bytes >= limit || ((int64_t)a.N + 1) > (limit - 1) / row_bytes)
    return fail(DPAC_EINVAL, "batch too large for one launch: every [N+1][B][d] array must stay "
                "below 2 GiB (B=%lld, N=%d, d=%d); split the batch over launches with "
                "traj_offset", (long long)a.B, a.N, a.eq.dim);
  return dispatch(a);
}

// dpac_policy_cost's launch: the lean kernels address no [N+1][B][d] array, and x0 / x_end only
// through descriptors over a workgroup's own rows; the limit is the [B][d] array's byte count in
// 32 bits.  dw, where it is given, is read through one descriptor like every [N][B][d] array.
int launch_lean(const OpArgs& a) {
  const int64_t esz = a.dtype == DPAC_F64 ? 8 : 4;
  if (a.eq.dim > (1 << 16)) return fail(DPAC_EINVAL, "dim %d too large", a.eq.dim);
  const int64_t row_bytes = a.B * a.eq.dim * esz;  // B <= 2^31, dim <= 2^16: no overflow
  if (row_bytes >= (int64_t)1 << 32)
    return fail(DPAC_EINVAL, "batch too large for one launch: a [B][d] array must stay below 4 GiB "
                "(B=%lld, d=%d); split the batch over launches with traj_offset", (long long)a.B, a.eq.dim);
  const int64_t limit = (int64_t)1 << 31;
  if (a.dw && (row_bytes >= limit || (int64_t)a.N > (limit - 1) / row_bytes))
    return fail(DPAC_EINVAL, "batch too large for one launch: the dw [N][B][d] array must stay below "
                "2 GiB (B=%lld, N=%d, d=%d); pass dw = NULL to draw the increments in-kernel, or split "
                "the batch over launches", (long long)a.B, a.N, a.eq.dim);
  return dispatch(a);
}

// The equation's elementwise sigma as (sa, sb) and k_td's lane split, for the fused
// TD1 entry points (TdRows, dpac_device.h; used by dpac_mlp_rows.h), after the checks the two
// share.  sigma and lanes come from the equation functors themselves (E::sigma_form, eqn_lanes),
// over an explicit allow-list of equation ids, so a new equation cannot reach the fused path
// with another's sigma.
int td_rows_setup(const dpac_eqn_params* eq, int32_t dtype, int64_t rows, const dpac_mlp* net,
                  const void* x, int64_t ldx, const void* u, const void* dw, TdRows& td) {
  if (int e = check_common(eq, dtype, rows)) return e;
  if (int e = check_net(net)) return e;
  if (net->ekn_head) return fail(DPAC_EINVAL, "the fused TD1 G network takes no Eikonal head");
  const int d = eq->dim;
  if (net->width[net->n_hidden + 1] != d)
    return fail(DPAC_EINVAL, "the network's output width (%d) must equal dim (%d)",
                net->width[net->n_hidden + 1], d);
  if (net->width[0] != d)
    return fail(DPAC_EINVAL, "the network's input width (%d) must equal dim (%d)", net->width[0], d);
  switch (eq->eqn) {  // the functor's template arguments do not enter sigma_form
    case DPAC_EQN_LQR: EqLQR<double, 1, 1>::sigma_form(*eq, td.sa, td.sb); break;
    case DPAC_EQN_LQR_VAR: EqLQRVar<double, 1, 1>::sigma_form(*eq, td.sa, td.sb); break;
    case DPAC_EQN_EKN: EqEKN<double, 1, 1>::sigma_form(*eq, td.sa, td.sb); break;
    case DPAC_EQN_VDP: EqVDP<double, 2, 1>::sigma_form(*eq, td.sa, td.sb); break;
    default: return fail(DPAC_EUNSUP, "no fused TD1 path for equation %d", eq->eqn);
  }
  td.p = eqn_lanes(eq->eqn, d);  // E::kP of the equation's k_td
  td.ldu = eq->control_dim;
  if (ldx < d) return fail(DPAC_EINVAL, "ldx (%lld) < dim (%d)", (long long)ldx, d);
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(dw);
  if (td.sb != 0.0) DPAC_REQUIRE(u);
  td.x = x; td.ldx = ldx; td.u = u; td.dw = dw;
  return DPAC_OK;
}

}  // namespace
}  // namespace dpac

using namespace dpac;

extern "C" {

int32_t dpac_abi_version(void) { return DPAC_ABI_VERSION; }

const char* dpac_last_error(void) { return g_err.c_str(); }

int32_t dpac_supported(const dpac_eqn_params* eq) { return check_eq(eq) == DPAC_OK ? 1 : 0; }

int dpac_sample(const dpac_eqn_params* eq, int32_t sample_type, int32_t dtype, int64_t num_sample,
                int32_t num_steps, uint64_t seed, int64_t traj_offset, void* x0, void* dw,
                void* x_bdry, void* stream) {
  if (!eq) return fail(DPAC_EINVAL, "eqn params pointer is NULL");
  if (int e = check_dtype(dtype)) return e;
  if (eq->dim < 1) return fail(DPAC_EINVAL, "dim must be >= 1");
  if (num_sample < 1) return fail(DPAC_EINVAL, "num_sample must be >= 1");
  if (dw && num_steps < 1) return fail(DPAC_EINVAL, "num_steps must be >= 1");
  if (int e = check_sample_type(sample_type)) return e;
  if (traj_offset < 0) return fail(DPAC_EINVAL, "traj_offset must be >= 0");
  const int r = sample_launch(dtype, eq, sample_type, num_sample, num_steps, seed, traj_offset, x0, dw,
                              x_bdry, (hipStream_t)stream);
  if (r) return fail(r, "sampler launch failed: %s", hipGetErrorString((hipError_t)r));
  return ok();
}

int dpac_rollout_fwd(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype, int64_t num_sample,
                     int32_t num_steps, double total_time, const void* x0, const void* dw,
                     uint64_t seed, int64_t traj_offset, int32_t sample_type, void* x, void* dt,
                     void* coef, void* u, int32_t cost_order, void* y, void* disc, void* stream) {
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  DPAC_REQUIRE(x0);
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(dt);
  DPAC_REQUIRE(coef);
  if ((y == nullptr) != (disc == nullptr))
    return fail(DPAC_EINVAL, "y and disc must both be given or both be NULL");
  if (int e = check_cost_order(cost_order)) return e;
  if (!dw) {
    if (int e = check_sample_type(sample_type)) return e;
    if (traj_offset < 0) return fail(DPAC_EINVAL, "traj_offset must be >= 0");
  }
  OpArgs a = blank(eq, OP_ROLLOUT, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.x0 = x0; a.dw = dw; a.seed = seed; a.traj_offset = traj_offset;
  a.sample_type = dw_sample_type(sample_type);
  a.x_out = x; a.dt = dt; a.coef = coef; a.u_out = u; a.cost_order = cost_order; a.y = y;
  a.disc = disc;
  return launch(a);
}

int32_t dpac_rollout_nn_mask_tile_bytes(const dpac_mlp* actor) {
  if (!actor || actor->n_hidden < 1 || actor->n_hidden > DPAC_MLP_MAX_HIDDEN) return 0;
  return nn_mask_tile_bytes(actor->n_hidden);
}

int64_t dpac_rollout_nn_mask_bytes(const dpac_mlp* actor, int32_t dtype, int64_t num_sample,
                                   int32_t num_steps) {
  if (!actor || actor->n_hidden < 1 || actor->n_hidden > DPAC_MLP_MAX_HIDDEN || num_sample < 1 ||
      num_steps < 1)
    return fail(DPAC_EINVAL, "dpac_rollout_nn_mask_bytes: bad arguments"), -1;
  if (check_dtype(dtype)) return -1;
  ok();
  // the same selection as run_op's OP_ROLLOUT_NN: float, 16-row tiles, the fast path
  if (dtype != DPAC_F32) return 0;
  const int tile = nn_tile_rows();
  if (tile == 4 || (tile == 0 && num_sample <= 1024)) return 0;
  const int L = actor->n_hidden;
  if (!nn_fast_host<float>(L, actor->width, actor->weight_km, actor->width[0], actor->width[L + 1]) &&
      !nn_x3_host(L, actor->width, actor->weight_x3, actor->width[0], actor->width[L + 1]))
    return 0;
  return (int64_t)num_steps * ((num_sample + 15) / 16) * nn_mask_tile_bytes(L);
}

int dpac_rollout_nn_fwd(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype,
                        int64_t num_sample, int32_t num_steps, double total_time,
                        const dpac_mlp* actor, const void* x0, const void* dw, void* x,
                        void* dt, void* coef, void* u, int32_t cost_order, void* y,
                        void* disc, void* save_z, int32_t* save_flag, void* save_disc,
                        uint8_t* save_mask, int32_t* mask_written, void* stream) {
  if (mask_written) *mask_written = 0;
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  if (int e = check_mlp(eq, actor)) return e;
  DPAC_REQUIRE(x0);
  DPAC_REQUIRE(dw);
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(dt);
  DPAC_REQUIRE(coef);
  if ((y == nullptr) != (disc == nullptr))
    return fail(DPAC_EINVAL, "y and disc must both be given or both be NULL");
  if (int e = check_cost_order(cost_order)) return e;
  const int nsave = (save_z != nullptr) + (save_flag != nullptr) + (save_disc != nullptr);
  if (nsave != 0 && nsave != 3)
    return fail(DPAC_EINVAL, "save_z, save_flag and save_disc must all be given or all be NULL");
  if (save_mask && nsave != 3) return fail(DPAC_EINVAL, "save_mask needs the other backward saves");
  OpArgs a = blank(eq, OP_ROLLOUT_NN, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.x0 = x0; a.dw = dw; a.mlp = *actor;
  a.x_out = x; a.dt = dt; a.coef = coef; a.u_out = u; a.cost_order = cost_order; a.y = y;
  a.disc = disc; a.save_z = save_z; a.save_flag = save_flag; a.save_disc = save_disc;
  a.save_mask = save_mask; a.mask_written = mask_written;
  return launch(a);
}

int dpac_policy_cost(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype, int64_t num_sample,
                     int32_t num_steps, double total_time, const dpac_mlp* actor, const void* x0,
                     const void* dw, uint64_t seed, int64_t traj_offset, int32_t sample_type,
                     int32_t cost_order, void* y, void* disc, void* x_end, void* tau, int32_t* steps,
                     void* stream) {
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  if (int e = check_mlp(eq, actor)) return e;
  DPAC_REQUIRE(x0);
  DPAC_REQUIRE(y);
  DPAC_REQUIRE(disc);
  DPAC_REQUIRE(x_end);
  if (int e = check_cost_order(cost_order)) return e;
  if (!dw) {
    if (int e = check_sample_type(sample_type)) return e;
    if (traj_offset < 0) return fail(DPAC_EINVAL, "traj_offset must be >= 0");
  }
  OpArgs a = blank(eq, OP_ROLLOUT_NN, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.x0 = x0; a.dw = dw; a.mlp = *actor; a.seed = seed; a.traj_offset = traj_offset;
  a.sample_type = dw_sample_type(sample_type);
  a.cost_order = cost_order; a.y = y; a.disc = disc; a.x_end = x_end; a.tau = tau; a.steps = steps;
  return launch_lean(a);
}

int dpac_rollout_nn_bwd(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype,
                        int64_t num_sample, int32_t num_steps, double total_time,
                        const dpac_mlp* actor, const void* const* weight_t,
                        const void* const* weight_t_km, const void* x,
                        const void* u, const void* dw, const void* save_z,
                        const int32_t* save_flag, const void* save_disc,
                        const uint8_t* save_mask, const void* g_xN,
                        const void* g_disc, const void* g_y, void* G, void* g_x0,
                        void* stream) {
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  if (int e = check_mlp(eq, actor)) return e;
  if (int e = check_weight_t(actor, weight_t)) return e;
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(u);
  DPAC_REQUIRE(dw);
  DPAC_REQUIRE(save_z);
  DPAC_REQUIRE(save_flag);
  DPAC_REQUIRE(save_disc);
  DPAC_REQUIRE(G);
  OpArgs a = blank(eq, OP_ROLLOUT_NN_BWD, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.mlp = backward_net(actor, weight_t_km);
  for (int i = 0; i <= actor->n_hidden; ++i) a.mlp_wt[i] = weight_t[i];
  a.x = x; a.u = u; a.dw = dw; a.save_z = const_cast<void*>(save_z);
  a.save_flag = const_cast<int32_t*>(save_flag); a.save_disc = const_cast<void*>(save_disc);
  a.g_x_out = g_xN; a.g_disc_out = g_disc; a.g_y_out = g_y; a.g_G = G; a.g_x = g_x0;
  a.mask_in = save_mask;
  return launch(a);
}

int64_t dpac_mlp_rows_mask_bytes(const dpac_mlp* net, int32_t dtype, int64_t rows) {
  if (check_net(net) || check_dtype(dtype) || check_rows(rows)) return -1;
  ok();
  return mlp_rows_mask_bytes(dtype, rows, *net);
}

int dpac_mlp_rows_fwd(int32_t dtype, int64_t rows, const dpac_mlp* net, const void* x,
                      int64_t ldx, void* out, void* save_z, uint8_t* save_mask,
                      int32_t* mask_written, void* stream) {
  if (mask_written) *mask_written = 0;
  if (int e = check_net(net)) return e;
  if (int e = check_dtype(dtype)) return e;
  if (int e = check_rows(rows)) return e;
  if (ldx < net->width[0]) return fail(DPAC_EINVAL, "ldx (%lld) < width[0] (%d)", (long long)ldx,
                                       net->width[0]);
  if (int e = check_weights(net)) return e;
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(out);
  if (save_mask && !save_z) return fail(DPAC_EINVAL, "save_mask needs save_z");
  return finish(mlp_rows_fwd_launch(dtype, rows, *net, x, ldx, out, save_z, nullptr, save_mask, mask_written,
                                    (hipStream_t)stream));
}

int dpac_mlp_rows_bwd(int32_t dtype, int64_t rows, const dpac_mlp* net, const void* const* weight_t,
                      const void* const* weight_t_km, const void* save_z, const uint8_t* save_mask,
                      const void* g_out, void* G, void* g_x, void* stream) {
  if (int e = check_net(net)) return e;
  if (int e = check_dtype(dtype)) return e;
  if (int e = check_rows(rows)) return e;
  if (int e = check_weight_t(net, weight_t)) return e;
  DPAC_REQUIRE(save_z);
  DPAC_REQUIRE(g_out);
  DPAC_REQUIRE(G);
  return finish(mlp_rows_bwd_launch(dtype, rows, backward_net(net, weight_t_km), weight_t, save_z, save_mask,
                                    g_out, G, g_x, nullptr, (hipStream_t)stream));
}

int dpac_mlp_rows_fwd_td1(const dpac_eqn_params* eq, int32_t dtype, int64_t rows, const dpac_mlp* net,
                          const void* x, int64_t ldx, const void* u, const void* dw, void* gdot,
                          void* save_z, uint8_t* save_mask, int32_t* mask_written, void* stream) {
  if (mask_written) *mask_written = 0;
  TdRows td{};
  if (int e = td_rows_setup(eq, dtype, rows, net, x, ldx, u, dw, td)) return e;
  if (int e = check_weights(net)) return e;
  DPAC_REQUIRE(gdot);
  if (save_mask && !save_z) return fail(DPAC_EINVAL, "save_mask needs save_z");
  td.gdot = gdot;
  return finish(mlp_rows_fwd_launch(dtype, rows, *net, x, ldx, nullptr, save_z, &td, save_mask, mask_written,
                                    (hipStream_t)stream));
}

int dpac_mlp_rows_bwd_td1(const dpac_eqn_params* eq, int32_t dtype, int64_t rows, const dpac_mlp* net,
                          const void* const* weight_t, const void* const* weight_t_km,
                          const void* save_z, const uint8_t* save_mask, const void* x, int64_t ldx,
                          const void* u, const void* dw, const void* g_gdot, void* G, void* g_x,
                          void* stream) {
  TdRows td{};
  if (int e = td_rows_setup(eq, dtype, rows, net, x, ldx, u, dw, td)) return e;
  if (int e = check_weight_t(net, weight_t)) return e;
  DPAC_REQUIRE(save_z);
  DPAC_REQUIRE(g_gdot);
  DPAC_REQUIRE(G);
  td.g_gdot = g_gdot;
  return finish(mlp_rows_bwd_launch(dtype, rows, backward_net(net, weight_t_km), weight_t, save_z, save_mask,
                                    nullptr, G, g_x, &td, (hipStream_t)stream));
}

int64_t dpac_mlp_param_grads_workspace(int32_t dtype, int64_t rows, const dpac_mlp* net) {
  if (check_net(net) || check_dtype(dtype) || check_rows(rows)) return -1;
  ok();
  return mlp_param_grads_ws_bytes(dtype, rows, *net);
}

int dpac_mlp_param_grads(int32_t dtype, int64_t rows, const dpac_mlp* net, double gamma_scale,
                         const void* x, int64_t ldx, const void* save_z, const void* G,
                         void* workspace, int64_t workspace_bytes, void* grads, void* stream) {
  if (int e = check_net(net)) return e;
  if (int e = check_dtype(dtype)) return e;
  if (int e = check_rows(rows)) return e;
  if (ldx < net->width[0]) return fail(DPAC_EINVAL, "ldx (%lld) < width[0] (%d)", (long long)ldx,
                                       net->width[0]);
  {
    int gtot = 0;
    for (int i = 0; i <= net->n_hidden + 1; ++i) gtot += net->width[i];
    if (ldx > gtot)
      return fail(DPAC_EINVAL, "ldx (%lld) must not exceed the G row width (%d)", (long long)ldx,
                  gtot);
  }
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(save_z);
  DPAC_REQUIRE(G);
  DPAC_REQUIRE(workspace);
  DPAC_REQUIRE(grads);
  const int64_t need = mlp_param_grads_ws_bytes(dtype, rows, *net);
  if (workspace_bytes < need)
    return fail(DPAC_EINVAL, "workspace too small: %lld bytes, need %lld",
                (long long)workspace_bytes, (long long)need);
  return finish(mlp_param_grads_launch(dtype, rows, *net, gamma_scale, x, ldx, save_z, G, workspace, grads,
                                       (hipStream_t)stream));
}

int dpac_flag_init(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype, int64_t num_sample,
                   int32_t num_steps, double total_time, const void* x0, int32_t* flag,
                   void* stream) {
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  DPAC_REQUIRE(x0);
  DPAC_REQUIRE(flag);
  OpArgs a = blank(eq, OP_FLAG_INIT, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.x0 = x0; a.flag_out = flag;
  return launch(a);
}

int dpac_step_fwd(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype, int64_t num_sample,
                  int32_t num_steps, double total_time, const void* x, const void* u,
                  const void* dw_t, const int32_t* flag_in, const void* disc_in, const void* y_in,
                  int32_t cost_order, void* x_out, int32_t* flag_out, void* disc_out, void* y_out,
                  void* dt, void* coef, void* stream) {
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(u);
  DPAC_REQUIRE(dw_t);
  DPAC_REQUIRE(flag_in);
  DPAC_REQUIRE(x_out);
  DPAC_REQUIRE(flag_out);
  if (x_out == x) return fail(DPAC_EINVAL, "x_out must not alias x");
  if (int e = check_cost_order(cost_order)) return e;
  OpArgs a = blank(eq, OP_STEP_FWD, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.x = x; a.u = u; a.dw = dw_t; a.flag_in = flag_in; a.disc_in = disc_in; a.y_in = y_in;
  a.cost_order = cost_order; a.x_out = x_out; a.flag_out = flag_out; a.disc_out = disc_out;
  a.y_out = y_out; a.dt = dt; a.coef = coef;
  return launch(a);
}

int dpac_step_bwd(const dpac_eqn_params* eq, int32_t scheme, int32_t dtype, int64_t num_sample,
                  int32_t num_steps, double total_time, const void* x, const void* u,
                  const void* dw_t, const int32_t* flag_in, const void* disc_in,
                  int32_t cost_order, const void* g_x_out, const void* g_disc_out,
                  const void* g_y_out, void* g_x, void* g_u, void* g_disc, void* stream) {
  if (int e = check_run(eq, scheme, dtype, num_sample, num_steps, total_time)) return e;
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(u);
  DPAC_REQUIRE(dw_t);
  DPAC_REQUIRE(flag_in);
  DPAC_REQUIRE(g_x_out);
  DPAC_REQUIRE(g_x);
  DPAC_REQUIRE(g_u);
  if (int e = check_cost_order(cost_order)) return e;
  OpArgs a = blank(eq, OP_STEP_BWD, scheme, dtype, num_sample, num_steps, total_time, stream);
  a.x = x; a.u = u; a.dw = dw_t; a.flag_in = flag_in; a.disc_in = disc_in;
  a.cost_order = cost_order; a.g_x_out = g_x_out; a.g_disc_out = g_disc_out;
  a.g_y_out = g_y_out; a.g_x = g_x; a.g_u = g_u; a.g_disc = g_disc;
  return launch(a);
}

// The TD entry points read a finished trajectory: no scheme, and T (unused) = 1.
int dpac_td_assemble_fwd(const dpac_eqn_params* eq, int32_t td_type, int32_t cost_order,
                         int32_t dtype, int64_t num_sample, int32_t num_steps, const void* x,
                         const void* u, const void* dw, uint64_t seed, int64_t traj_offset,
                         int32_t sample_type, const void* dt, const void* coef, const void* G,
                         void* y, void* disc, void* stream) {
  if (int e = check_common(eq, dtype, num_sample)) return e;
  if (num_steps < 1) return fail(DPAC_EINVAL, "num_steps must be >= 1");
  if (td_type != DPAC_TD1 && td_type != DPAC_TD2 && td_type != DPAC_TD1_GDOT)
    return fail(DPAC_EINVAL, "bad td_type %d", td_type);
  if (int e = check_cost_order(cost_order)) return e;
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(u);
  DPAC_REQUIRE(dt);
  DPAC_REQUIRE(coef);
  DPAC_REQUIRE(y);
  DPAC_REQUIRE(disc);
  if (td_type == DPAC_TD1) {
    DPAC_REQUIRE(G);
    if (!dw) {
      if (int e = check_sample_type(sample_type)) return e;
    }
  }
  if (td_type == DPAC_TD1_GDOT) DPAC_REQUIRE(G);  // gdot [N][B]; dw is not read
  OpArgs a = blank(eq, OP_TD_FWD, 0, dtype, num_sample, num_steps, 1.0, stream);
  a.td_type = td_type; a.cost_order = cost_order; a.x = x; a.u = u; a.dw = dw; a.seed = seed;
  a.traj_offset = traj_offset;
  a.sample_type = dw_sample_type(sample_type);
  a.dt_in = dt; a.coef_in = coef; a.G = G; a.y = y; a.disc = disc;
  return launch(a);
}

int dpac_td_assemble_bwd(const dpac_eqn_params* eq, int32_t dtype, int64_t num_sample,
                         int32_t num_steps, const void* x, const void* u, const void* dw,
                         uint64_t seed, int64_t traj_offset, int32_t sample_type, const void* dt,
                         const void* coef, const void* g_y, void* g_G, void* stream) {
  if (int e = check_common(eq, dtype, num_sample)) return e;
  if (num_steps < 1) return fail(DPAC_EINVAL, "num_steps must be >= 1");
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(u);
  DPAC_REQUIRE(dt);
  DPAC_REQUIRE(coef);
  DPAC_REQUIRE(g_y);
  DPAC_REQUIRE(g_G);
  if (!dw) {
    if (int e = check_sample_type(sample_type)) return e;
  }
  OpArgs a = blank(eq, OP_TD_BWD, 0, dtype, num_sample, num_steps, 1.0, stream);
  a.x = x; a.u = u; a.dw = dw; a.seed = seed; a.traj_offset = traj_offset;
  a.sample_type = dw_sample_type(sample_type);
  a.dt_in = dt; a.coef_in = coef; a.g_y_out = g_y; a.g_G = g_G;
  return launch(a);
}

int dpac_td_assemble_bwd_gdot(const dpac_eqn_params* eq, int32_t dtype, int64_t num_sample,
                              int32_t num_steps, const void* dt, const void* coef, const void* g_y,
                              void* g_gdot, void* stream) {
  if (int e = check_common(eq, dtype, num_sample)) return e;
  if (num_steps < 1) return fail(DPAC_EINVAL, "num_steps must be >= 1");
  DPAC_REQUIRE(dt);
  DPAC_REQUIRE(coef);
  DPAC_REQUIRE(g_y);
  DPAC_REQUIRE(g_gdot);
  OpArgs a = blank(eq, OP_TD_BWD, 0, dtype, num_sample, num_steps, 1.0, stream);
  a.td_type = DPAC_TD1_GDOT; a.dt_in = dt; a.coef_in = coef; a.g_y_out = g_y; a.g_G = g_gdot;
  return launch(a);
}

int dpac_actor_cost_fwd(const dpac_eqn_params* eq, int32_t dtype, int64_t num_sample,
                        int32_t num_steps, const void* x, const void* u, const void* dt,
                        const void* coef, void* y, void* disc, void* stream) {
  return dpac_td_assemble_fwd(eq, DPAC_TD2, DPAC_COST_ACTOR, dtype, num_sample, num_steps, x, u,
                              nullptr, 0, 0, DPAC_SAMPLE_NORMAL, dt, coef, nullptr, y, disc, stream);
}

int dpac_equation_eval(const dpac_eqn_params* eq, int32_t what, int32_t dtype, int64_t num_sample,
                       const void* x, const void* u, void* out, void* stream) {
  if (int e = check_common(eq, dtype, num_sample)) return e;
  if (what < DPAC_EVAL_DRIFT || what > DPAC_EVAL_B) return fail(DPAC_EINVAL, "bad eval id %d", what);
  DPAC_REQUIRE(x);
  DPAC_REQUIRE(out);
  if ((what == DPAC_EVAL_DRIFT || what == DPAC_EVAL_SIGMA || what == DPAC_EVAL_W) && !u)
    return fail(DPAC_EINVAL, "eval %d needs u", what);
  OpArgs a = blank(eq, OP_EVAL, 0, dtype, num_sample, 1, 1.0, stream);
  a.what = what; a.x = x; a.u = u; a.out = out;
  return launch(a);
}

int dpac_mlp_prepare(int32_t dtype, const dpac_mlp* net, double gamma_scale, void* scales,
                     void* weight_t, void* weight_km, void* weight_t_km, void* weight_x3,
                     void* weight_t_x3, void* stream) {
  if (int e = check_net(net)) return e;
  if (int e = check_dtype(dtype)) return e;
  DPAC_REQUIRE(scales);
  if ((weight_x3 || weight_t_x3) && dtype != DPAC_F32)
    return fail(DPAC_EINVAL, "split-fp16 images (weight_x3 / weight_t_x3) are float-only");
  if (weight_t || weight_km || weight_t_km || weight_x3 || weight_t_x3)
    if (int e = check_weights(net)) return e;
  return finish(mlp_prepare_launch(dtype, *net, gamma_scale, scales, weight_t, weight_km, weight_t_km,
                                   weight_x3, weight_t_x3, (hipStream_t)stream));
}

int dpac_adam_apply(int32_t dtype, int32_t n_tensors, const int64_t* numel, void* const* var,
                    const void* const* grad, void* const* m, void* const* v, double alpha,
                    double beta_1, double beta_2, double epsilon, void* stream) {
  if (int e = check_adam_tensors(dtype, n_tensors, numel, var, grad, m, v)) return e;
  if (n_tensors == 0) return ok();
  return finish(adam_launch(dtype, n_tensors, numel, var, grad, m, v, alpha, beta_1, beta_2, epsilon,
                            (hipStream_t)stream));
}

int dpac_adam_step(int32_t dtype, int32_t n_tensors, const int64_t* numel, void* const* var,
                   const void* const* grad, void* const* m, void* const* v, dpac_adam_state* state,
                   const void* alpha_table, int64_t table_len, double beta_1, double beta_2,
                   double epsilon, int32_t advance, void* stream) {
  if (int e = check_adam_tensors(dtype, n_tensors, numel, var, grad, m, v)) return e;
  DPAC_REQUIRE(state);
  DPAC_REQUIRE(alpha_table);
  if (table_len < 1) return fail(DPAC_EINVAL, "table_len must be >= 1 (got %lld)", (long long)table_len);
  if (n_tensors == 0 && !advance) return ok();
  return finish(adam_step_launch(dtype, n_tensors, numel, var, grad, m, v, state, alpha_table, table_len,
                                 beta_1, beta_2, epsilon, advance, (hipStream_t)stream));
}

int dpac_critic_loss_grad(int32_t dtype, int64_t num_sample, const void* V, const void* y, const void* disc,
                          const void* z_bdry, double scale, double delta_clip, void* g_out, void* neg_g,
                          void* stream) {
  if (int e = check_dtype(dtype)) return e;
  if (num_sample < 1) return fail(DPAC_EINVAL, "num_sample must be >= 1 (got %lld)", (long long)num_sample);
  if (!(delta_clip > 0)) return fail(DPAC_EINVAL, "delta_clip must be > 0");
  DPAC_REQUIRE(V);
  DPAC_REQUIRE(y);
  DPAC_REQUIRE(disc);
  DPAC_REQUIRE(z_bdry);
  DPAC_REQUIRE(g_out);
  DPAC_REQUIRE(neg_g);
  return finish(critic_loss_launch(dtype, num_sample, V, y, disc, z_bdry, scale, delta_clip, g_out, neg_g,
                                   (hipStream_t)stream));
}

}  // extern "C"
