/* smpc_fixed_shapes.h — the switch and the query of the fixed-shape kernels, beside include/smpc.h (whose list of
 * functions is unchanged). Same library, same handle, same error codes. */
#ifndef SMPC_FIXED_SHAPES_H
#define SMPC_FIXED_SHAPES_H

#include "smpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fixed-shape kernels. For the shapes the library lists (csrc/smpc_launch.hpp, SMPC_FIXED_SHAPES: the headline
 * configuration, control_horizon 18 / parameter_block_length 6 at T = 28 with N = 8) the solve and K1 kernels are also
 * compiled with T, N, the control horizon and the block length as constants; a launch of such a shape runs them instead
 * of the kernels that take the shape as launch values, with the same results bit for bit. smpc_set_fixed_shapes(h, 0)
 * turns that off for this handle, (h, 1) on again (the default); it is read at every launch.
 * smpc_solve_shape_is_fixed: 1 if a plain smpc_solve_batch of B scenes with T rollout steps and N agents on this handle
 * (no T_scene, no scene_params: those, like smpc_solve_trace_batch, always run the general kernels) runs a fixed-shape
 * kernel, else 0 — a shape that is not listed, the one-scene-per-wave kernel of a small batch (smpc_solve_slot_width),
 * fixed shapes turned off. A function of its arguments and the handle alone. Negative smpc_error as for
 * smpc_solve_slot_width. */
int smpc_set_fixed_shapes(smpc_handle* h, int32_t enable);
int smpc_solve_shape_is_fixed(const smpc_handle* h, int32_t B, int32_t T, int32_t N);
/* The same for a plain smpc_eval_batch (K1) with T rollout steps and N agents: its slot width does not depend on B. */
int smpc_eval_shape_is_fixed(const smpc_handle* h, int32_t T, int32_t N);

#ifdef __cplusplus
}
#endif

#endif
