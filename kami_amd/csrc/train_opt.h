// train_opt.h — the trainer's step with kh_train_config's optimizer options (momentum, Nesterov, L2 decay, gradient-norm
// clipping; include/kami_hip.h states the rule).  kh_internal.h's train_step stays the reference's plain SGD step;
// train_step_opt is the same forward and backward with the fused update of train.hip's opt_update_kernel behind it.
#pragma once

#include "kh_internal.h"

namespace kh {

// the update rule of one step: kh_train_config's lr and optimizer fields
struct StepOpt {
    float lr, momentum, weight_decay, max_grad_norm;
    int nesterov;
    bool plain() const { return momentum == 0.0f && weight_decay == 0.0f && max_grad_norm == 0.0f && nesterov == 0; }
    bool operator==(const StepOpt& o) const
    {
        return lr == o.lr && momentum == o.momentum && weight_decay == o.weight_decay && max_grad_norm == o.max_grad_norm && nesterov == o.nesterov;
    }
};
// vel: the blob-shaped velocity (read and written with momentum > 0); norm_part: train_norm_parts() doubles (written with
// max_grad_norm > 0); frozen: train_frozen_ranges() in device memory
struct OptBuffers { float* vel; double* norm_part; const long long* frozen; };
// floats of one step's result block: [2 B] loss rows, 2 ints (NaN flags of the forward's outputs), then — written by
// train_step_opt with max_grad_norm > 0 only — the gradient norm before clipping and the clip factor c
constexpr size_t train_result_floats(int B) { return (size_t)B * 2 + 4; }
// the blob's BatchNorm running-statistics slots as ascending, disjoint float ranges [lo, hi): 2 * count values
size_t train_frozen_ranges(const TrainNet& n, const long long** ranges);
size_t train_norm_parts(size_t blob_floats);
hipError_t train_step_opt(const TrainNet& n, const StepBuffers& sb, const OptBuffers& ob, const float* x_in, const float* obsp,
                          const float* obsv, int B, const StepOpt& opt, float* loss_rows /* train_result_floats(B) */, hipStream_t s);

}  // namespace kh
