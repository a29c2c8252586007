// The Yogi step of the online fit as ONE kernel over a flat parameter / gradient / moment buffer (model/yogi.py:39-90).
//
// The reference's step is, per parameter tensor, eight elementwise tensor operations (yogi.py:69-88); on the device that is
// 12 parameters x 8 launches per iteration of a 478 342-parameter net on a batch of 1 024 - the fit was launch-bound (r05:
// 2.3 ms an iteration, 57 % of the online loop's wall-clock).  Here: the same operations per element in the same order, fp32
// where the reference's tensor operations are fp32 (a Python scalar enters a float32 tensor operation as a float), no
// contraction (the library is built with -ffp-contract=off), one launch; the step count and the powers of the betas live on
// the device (advanced by a one-thread kernel in front), so that an iteration is the same sequence of launches every time and
// can be replayed from a HIP graph (tetris_mcts_amd/train.py).
//   state (doubles): [0] step t, [1] beta1^t, [2] beta2^t, [3] lr / (1 - beta1^t), [4] sqrt(1 - beta2^t)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/tetris_mcts_hip.h"
#include "fit_mma.h"      // block_sum, up4: the fixed-order sums of the fit's kernels

namespace tmcts {

__global__ void k_yogi_tick(double* st, double lr, double b1, double b2) {
    const double t = st[0] + 1.0;
    const double p1 = t == 1.0 ? b1 : st[1] * b1, p2 = t == 1.0 ? b2 : st[2] * b2;
    st[0] = t; st[1] = p1; st[2] = p2;
    st[3] = lr / (1.0 - p1);            // step_size = lr / bias_correction1              (yogi.py:84-85)
    st[4] = sqrt(1.0 - p2);             // math.sqrt(bias_correction2)                     (yogi.py:82)
}

__global__ __launch_bounds__(256) void k_yogi_step(float* __restrict__ p, const float* __restrict__ g_, float* __restrict__ m,
                                                   float* __restrict__ v, const double* __restrict__ st, int n, float b1, float omb1,
                                                   float nomb2, float eps, float wd) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool first = st[0] == 1.0;
    const float step = (float)st[3], bc2 = (float)st[4];
    float g = g_[i];
    const float pi = p[i];
    float mi = first ? 0.f : m[i];                        // exp_avg = zeros, exp_avg_sq = grad * grad       (yogi.py:62-66)
    float vi = first ? g * g : v[i];
    if (wd != 0.f) g = g + wd * pi;                       // grad.add(p, alpha=weight_decay)                 (yogi.py:69-70)
    mi = mi * b1;                                         // exp_avg.mul_(beta1)
    mi = mi + omb1 * g;                                   //        .add_(grad, alpha=1 - beta1)             (yogi.py:73)
    const float g2 = g * g;                               // grad.mul(grad)
    const float d = vi - g2;
    const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : d;  // torch.sign (0 stays 0, NaN stays NaN)
    vi = vi + (nomb2 * sg) * g2;                          // exp_avg_sq.addcmul_(sign, grad_squared, value=-(1 - beta2))   (yogi.py:75-78)
    const float den = sqrtf(vi) / bc2 + eps;              // (exp_avg_sq.sqrt() / math.sqrt(bias_correction2)).add_(eps)  (yogi.py:82)
    p[i] = pi + (-step * mi) / den;                       // p.addcdiv_(exp_avg, denom, value=-step_size)    (yogi.py:87)
    m[i] = mi;
    v[i] = vi;
}

// torch.optim.Adam's single-tensor step (torch 2.10, not capturable), fp32 per element in its order of operations; the state is
// the one k_yogi_tick advances.
__global__ __launch_bounds__(256) void k_adam_step(float* __restrict__ p, const float* __restrict__ g_, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ vmax, const double* __restrict__ st,
                                                   int n, float omb1, float b2, float omb2, float eps, float wd, int amsgrad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float step = (float)st[3], bc2 = (float)st[4];
    float g = g_[i];
    const float pi = p[i];
    if (wd != 0.f) g = g + wd * pi;                       // grad.add(param, alpha=weight_decay)
    float mi = m[i];
    mi = mi + omb1 * (g - mi);                            // exp_avg.lerp_(grad, 1 - beta1)          (weight < 0.5: start + w (end - start))
    float vi = v[i] * b2;                                 // exp_avg_sq.mul_(beta2)
    vi = vi + (omb2 * g) * g;                             //           .addcmul_(grad, grad, value=1 - beta2)
    float dv = vi;
    if (amsgrad) {
        const float vm = vmax[i];
        dv = (vm != vm || vm > vi) ? vm : vi;             // torch.maximum(max_exp_avg_sq, exp_avg_sq) (NaN propagates)
        vmax[i] = dv;
    }
    const float den = sqrtf(dv) / bc2 + eps;              // (sqrt / bias_correction2_sqrt).add_(eps)
    p[i] = pi + (-step * mi) / den;                       // param.addcdiv_(exp_avg, denom, value=-step_size)
    m[i] = mi;
    v[i] = vi;
}

// ---- the penalty of elastic weight consolidation over the flat buffers (tm_ewc_penalty) ----
// Per element, in float, in this order: d = p - anchor, t = (lam F) d, grad = grad + t.  A workgroup's share of the loss,
// sum F d d in double (F and the float d converted first), goes to part[block] in block_sum's fixed order.
constexpr int EWC_BLOCK = 256;

__global__ __launch_bounds__(256) void k_ewc_penalty(const float* __restrict__ p, const float* __restrict__ anchor,
                                                     const float* __restrict__ fisher, int n, float lam, float* __restrict__ grad,
                                                     double* __restrict__ part) {
    __shared__ double sm[256];
    const int i = blockIdx.x * EWC_BLOCK + threadIdx.x;
    double s = 0.0;
    if (i < n) {
        const float f = fisher[i], d = p[i] - anchor[i];
        const float t = (lam * f) * d;
        grad[i] = grad[i] + t;
        s = ((double)f * (double)d) * (double)d;
    }
    s = tmcts_fit::block_sum(s, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// loss[0] = 0.5 lam (the sum of the S partials: thread t adds part[t], part[t + 256], ... in ascending order, then block_sum)
__global__ __launch_bounds__(256) void k_ewc_loss(const double* __restrict__ part, int S, double lam, double* __restrict__ loss) {
    __shared__ double sm[256];
    double s = 0.0;
    for (int k = threadIdx.x; k < S; k += 256) s += part[k];
    s = tmcts_fit::block_sum(s, sm);
    if (threadIdx.x == 0) loss[0] = (0.5 * lam) * s;
}

}  // namespace tmcts

extern "C" long long tm_ewc_penalty_workspace(int n) {
    if (n < 1) return -1;
    const long long blocks = ((long long)n + tmcts::EWC_BLOCK - 1) / tmcts::EWC_BLOCK;
    return tmcts_fit::up4(2 * blocks);      // one double a workgroup, in floats
}

extern "C" int tm_ewc_penalty(const float* p, const float* anchor, const float* fisher, int n, double lambda, float* grad, double* loss,
                              float* workspace, void* stream) {
    if (!p || !anchor || !fisher || !grad || !loss || !workspace || n < 1) return (int)hipErrorInvalidValue;
    if (!(lambda >= 0.0) || !isfinite(lambda) || ((uintptr_t)workspace & 15) || ((uintptr_t)loss & 7)) return (int)hipErrorInvalidValue;
    const int blocks = (int)(((long long)n + tmcts::EWC_BLOCK - 1) / tmcts::EWC_BLOCK);
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(tmcts::k_ewc_penalty, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, anchor, fisher, n, (float)lambda, grad, part);
    hipLaunchKernelGGL(tmcts::k_ewc_loss, dim3(1), dim3(256), 0, (hipStream_t)stream, part, blocks, lambda, loss);
    return (int)hipGetLastError();
}

extern "C" int tm_adam_step(float* p, const float* g, float* m, float* v, float* vmax, double* state, int n, double lr, double beta1,
                            double beta2, double eps, double weight_decay, int amsgrad, void* stream) {
    if (!p || !g || !m || !v || !vmax || !state || n < 0 || !(beta1 > 0.5)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tmcts::k_yogi_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, state, lr, beta1, beta2);
    if (n > 0)
        hipLaunchKernelGGL(tmcts::k_adam_step, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, g, m, v, vmax, state, n,
                           (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, amsgrad);
    return (int)hipGetLastError();
}

extern "C" int tm_yogi_step(float* p, const float* g, float* m, float* v, double* state, int n, double lr, double beta1, double beta2,
                            double eps, double weight_decay, void* stream) {
    if (!p || !g || !m || !v || !state || n < 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(tmcts::k_yogi_tick, dim3(1), dim3(1), 0, (hipStream_t)stream, state, lr, beta1, beta2);
    if (n > 0)
        hipLaunchKernelGGL(tmcts::k_yogi_step, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, g, m, v, state, n,
                           (float)beta1, (float)(1.0 - beta1), (float)(-(1.0 - beta2)), (float)eps, (float)weight_decay);      // (Python scalars: doubles, float32 in the tensor operation)
    return (int)hipGetLastError();
}
