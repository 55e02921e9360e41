// dpac_host.h — the host launchers that cross translation units: defined in dpac_mlp.hip,
// dpac_params.hip and dpac_sample.hip, called from dpac_abi.hip after it has validated the
// arguments.  Definer and caller both include this header, so a drifting signature does not
// compile.  Each returns 0 or the hipError_t of the failed launch.  (register_dispatch /
// find_dispatch, the equation TUs' table, are declared in dpac_launch.h.)
#pragma once
#include "dpac_device.h"

namespace dpac {
// dpac_mlp.hip
int64_t mlp_param_grads_ws_bytes(int dtype, int64_t rows, const dpac_mlp& net);
int mlp_param_grads_launch(int dtype, int64_t rows, const dpac_mlp& net, double gamma_scale,
                           const void* x, int64_t ldx, const void* z, const void* G, void* ws,
                           void* out, hipStream_t s);
int mlp_rows_fwd_launch(int dtype, int64_t rows, const dpac_mlp& net, const void* x, int64_t ldx,
                        void* out, void* save_z, const TdRows* td, uint8_t* mask, int32_t* written,
                        hipStream_t s);
int mlp_rows_bwd_launch(int dtype, int64_t rows, const dpac_mlp& net, const void* const* wt,
                        const void* save_z, const uint8_t* mask, const void* g_out, void* G, void* g_x,
                        const TdRows* td, hipStream_t s);
int64_t mlp_rows_mask_bytes(int dtype, int64_t rows, const dpac_mlp& net);
// dpac_params.hip
int mlp_prepare_launch(int dtype, const dpac_mlp& net, double gamma_scale, void* scales, void* wt,
                       void* wkm, void* wtkm, void* wx3, void* wtx3, hipStream_t s);
int critic_loss_launch(int dtype, int64_t B, const void* V, const void* y, const void* disc, const void* zb,
                       double scale, double clip, void* g_out, void* neg_g, hipStream_t s);
int adam_launch(int dtype, int n, const int64_t* numel, void* const* var, const void* const* grad,
                void* const* m, void* const* v, double alpha, double b1, double b2, double eps,
                hipStream_t s);
int adam_step_launch(int dtype, int n, const int64_t* numel, void* const* var, const void* const* grad,
                     void* const* m, void* const* v, dpac_adam_state* state, const void* table,
                     int64_t table_len, double b1, double b2, double eps, int advance, hipStream_t s);
// dpac_sample.hip: dpac_sample's launches (x0, dw, x_bdry: any may be NULL)
int sample_launch(int dtype, const dpac_eqn_params* eq, int32_t sample_type, int64_t B, int32_t N,
                  uint64_t seed, int64_t traj_offset, void* x0, void* dw, void* x_bdry, hipStream_t s);
}  // namespace dpac
