// k_optim.h — the optimizer step and the weight EMA of a training step over ONE flat arena (achelous_amd/optim.py FusedOptimizer; the reference's
// optimizer.step() + ema.update(model), utils/utils_fit.py:117-118,164-174, loss/detection_loss.py:449-459).
//
// Layout (built by the host, optim.py): four fp32 arenas.  `state` = [group 0 | group 1 | group 2 | parameters in no group | float buffers], `ema` the same;
// `grad`, `m1` (momentum buffer / exp_avg) and `m2` (exp_avg_sq) cover the parameter part only.  Every tensor starts at a multiple of OPT_CHUNK = 256 elements, so a
// chunk belongs to exactly one tensor, a wave owns a chunk (64 lanes x one 16-byte access) and every index a kernel forms is chunk * 256 + lane * 4 with
// chunk < chunks — a count the host derived from the arena's own numel().  No pointer table, no indirection: flags[chunk] and t[chunk] are indexed by the chunk itself.
//   flags[chunk]  bits 0-2: 0 / 1 / 2 the parameter group, 3 a parameter in no group (never optimised), 4 a float buffer; bit 3 (OPT_ACTIVE): the parameter has a
//                 gradient this step.  A chunk that is not active is not touched by the update rule — no decay, no momentum — as torch skips a parameter without .grad.
//   t[chunk]      Adam: the steps this chunk's parameter has taken (per parameter, as torch keeps it).
//   hyper         doubles: lr[3], weight_decay[3], ema_decay, ema_tau, updates, d.  The ONLY place a learning rate is read from, so a replayed graph sees the value
//                 the host wrote last.
// Padding elements are zero in every arena and stay zero under every rule here (0 gradient, 0 moments: every update of a zero by zeros is a zero).
#pragma once
#include "ach_platform.h"

namespace ach {

constexpr int OPT_CHUNK = 256;                 // elements per chunk = 64 lanes x 4
constexpr int OPT_ACTIVE = 8;
constexpr int OPT_SGD = 0, OPT_ADAM = 1, OPT_ADAMW = 2;
constexpr int OPT_LR = 0, OPT_WD = 3, OPT_EMA_DECAY = 6, OPT_EMA_TAU = 7, OPT_UPDATES = 8, OPT_D = 9, OPT_HYPER = 10;

// ModelEMA.update's first two lines (detection_loss.py:452-453) in double, on the device: updates += 1; d = decay * (1 - exp(-updates / tau))
static __global__ __launch_bounds__(64) void optim_tick_kernel(double* hyper) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double u = hyper[OPT_UPDATES] + 1.0;
        hyper[OPT_UPDATES] = u;
        hyper[OPT_D] = hyper[OPT_EMA_DECAY] * (1.0 - exp(-u / hyper[OPT_EMA_TAU]));
    }
}

struct OptimStepParams {
    float* state; float* ema; const float* grad; float* m1; float* m2;
    const int* flags; int* t; const double* hyper;
    int chunks, pchunks, kind, nesterov;
    float mu;                       // SGD momentum
    double beta1, beta2, eps;       // Adam
};

// torch.lerp_(end, w) for a float weight: the formula ATen picks by the weight's size
__device__ __forceinline__ float optim_lerp(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w); }

// one element of torch.optim.SGD._single_tensor_sgd (dampening 0; a zero buffer makes the first step buf = g)
__device__ __forceinline__ float optim_sgd(float p, float g, float& buf, float lr, float wd, float mu, bool has_buf, bool nesterov) {
    if (wd != 0.0f) g = g + wd * p;
    if (has_buf) {
        buf = buf * mu + g;
        g = nesterov ? g + mu * buf : buf;
    }
    return p - lr * g;
}
// one element of torch.optim.Adam / AdamW._single_tensor_adam: step = lr / (1 - beta1^t), bc2s = sqrt(1 - beta2^t), both from the host-precision doubles
__device__ __forceinline__ float optim_adam(float p, float g, float& m, float& v, float lr_wd, float wd, bool decoupled, float w1, float beta2, float w2, float bc2s,
                                            float eps, float step) {
    if (decoupled) p = p * (1.0f - lr_wd);
    else if (wd != 0.0f) g = g + wd * p;
    m = optim_lerp(m, g, w1);
    v = v * beta2 + w2 * g * g;
    const float denom = sqrtf(v) / bc2s + eps;
    return p - step * (m / denom);
}

// grid-stride over chunks, one wave per chunk and iteration; a workgroup is four waves
static __global__ __launch_bounds__(256) void optim_step_kernel(const OptimStepParams q) {
    const int lane = int(threadIdx.x) & 63, wave = int(threadIdx.x) >> 6;
    const bool has_ema = q.ema != nullptr;
    float d = 0.0f, omd = 0.0f;
    if (has_ema) {                                                // the reference multiplies by the Python floats d and (1 - d): each rounded to float32 once
        const double dd = q.hyper[OPT_D];
        d = float(dd); omd = float(1.0 - dd);
    }
    for (long c = long(blockIdx.x) * 4 + wave; c < long(q.chunks); c += long(gridDim.x) * 4) {
        const long at = c * OPT_CHUNK + lane * 4;
        const int flag = c < long(q.pchunks) ? q.flags[c] : 4;
        const int gid = flag & 7;
        float4 p = *reinterpret_cast<const float4*>(q.state + at);
        if (gid <= 2 && (flag & OPT_ACTIVE)) {                    // wave-uniform: a chunk has one flag
            const float4 g = *reinterpret_cast<const float4*>(q.grad + at);
            const double lr = q.hyper[OPT_LR + gid], wd = q.hyper[OPT_WD + gid];
            if (q.kind == OPT_SGD) {
                const bool has_buf = q.mu != 0.0f;
                float4 b = has_buf ? *reinterpret_cast<const float4*>(q.m1 + at) : make_float4(0.f, 0.f, 0.f, 0.f);
                p.x = optim_sgd(p.x, g.x, b.x, float(lr), float(wd), q.mu, has_buf, q.nesterov != 0);
                p.y = optim_sgd(p.y, g.y, b.y, float(lr), float(wd), q.mu, has_buf, q.nesterov != 0);
                p.z = optim_sgd(p.z, g.z, b.z, float(lr), float(wd), q.mu, has_buf, q.nesterov != 0);
                p.w = optim_sgd(p.w, g.w, b.w, float(lr), float(wd), q.mu, has_buf, q.nesterov != 0);
                if (has_buf) *reinterpret_cast<float4*>(q.m1 + at) = b;
            } else {
                // every lane reads the count, lane 0 writes it back AFTER all have (the lane read is the wave's meeting point)
                const int steps = wave_lane_i32(q.t[c], 0) + 1;
                if (lane == 0) q.t[c] = steps;
                const double bc1 = 1.0 - pow(q.beta1, double(steps)), bc2 = 1.0 - pow(q.beta2, double(steps));
                const float step = float(lr / bc1), bc2s = float(sqrt(bc2));
                const float w1 = float(1.0 - q.beta1), w2 = float(1.0 - q.beta2), lr_wd = float(lr * wd);
                float4 m = *reinterpret_cast<const float4*>(q.m1 + at), v = *reinterpret_cast<const float4*>(q.m2 + at);
                const bool dec = q.kind == OPT_ADAMW;
                p.x = optim_adam(p.x, g.x, m.x, v.x, lr_wd, float(wd), dec, w1, float(q.beta2), w2, bc2s, float(q.eps), step);
                p.y = optim_adam(p.y, g.y, m.y, v.y, lr_wd, float(wd), dec, w1, float(q.beta2), w2, bc2s, float(q.eps), step);
                p.z = optim_adam(p.z, g.z, m.z, v.z, lr_wd, float(wd), dec, w1, float(q.beta2), w2, bc2s, float(q.eps), step);
                p.w = optim_adam(p.w, g.w, m.w, v.w, lr_wd, float(wd), dec, w1, float(q.beta2), w2, bc2s, float(q.eps), step);
                *reinterpret_cast<float4*>(q.m1 + at) = m;
                *reinterpret_cast<float4*>(q.m2 + at) = v;
            }
            *reinterpret_cast<float4*>(q.state + at) = p;
        }
        if (has_ema) {                                            // v *= d; v += (1 - d) * x, x the value after the update (detection_loss.py:456-459)
            float4 e = *reinterpret_cast<const float4*>(q.ema + at);
            e.x = e.x * d + omd * p.x;
            e.y = e.y * d + omd * p.y;
            e.z = e.z * d + omd * p.z;
            e.w = e.w * d + omd * p.w;
            *reinterpret_cast<float4*>(q.ema + at) = e;
        }
    }
}

}  // namespace ach
