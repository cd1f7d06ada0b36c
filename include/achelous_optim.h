/* achelous_optim.h — extension of the C ABI of libachelous_hip.so (include/achelous.h, which this header includes and whose conventions, error codes and
 * ach_last_error(NULL) it shares): the optimizer step and the weight EMA of a training step over one flat training-state arena.  A header of its own, so that the
 * set of entries include/achelous.h declares stays what it is; the Python binding reads this header exactly as it reads that one (achelous_amd/engine.py
 * OPTIM_ENTRIES; achelous_amd/optim.py FusedOptimizer builds the arenas). */
#ifndef ACHELOUS_OPTIM_H_
#define ACHELOUS_OPTIM_H_

#include "achelous.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Both entries are stateless, launch on `stream` and synchronise nothing.  Every buffer is the caller's, on the device, float32 unless said otherwise.
 *   Arenas.  `state` and `ema` hold `chunks` chunks of 256 elements: [group 0 | group 1 | group 2 | parameters in no group | float buffers]; `grad`, `m1` (momentum
 *   buffer / exp_avg) and `m2` (exp_avg_sq) hold the first `param_chunks` of them.  Every tensor starts at a chunk boundary; padding is zero and stays zero.  All 16-byte
 *   aligned.  The kernels form no address but chunk * 256 + lane * 4 with chunk < chunks (< param_chunks for grad, m1, m2, t).
 *   flags  int32 [chunks]: bits 0-2 = 0 / 1 / 2 the parameter group, 3 a parameter that is never optimised, 4 a float buffer; bit 3 (value 8): the parameter has a
 *          gradient this step.  Chunks at or behind param_chunks are buffers whatever their flag says.
 *   t      int32 [param_chunks]: Adam's step count of the chunk's parameter; incremented for every active chunk.  NULL for sgd.
 *   hyper  double [10]: 0-2 lr of the groups, 3-5 their weight_decay, 6 ema_decay, 7 ema_tau, 8 updates, 9 d.
 *
 * ach_optim_tick: updates += 1; d = ema_decay * (1 - exp(-updates / ema_tau)), in double (the reference's ModelEMA.update, loss/detection_loss.py:452-453).
 *
 * ach_optim_step, one launch over all chunks.  An ACTIVE chunk of group g: kind 0 = torch.optim.SGD (g += wd p; momentum != 0: buf = momentum buf + g, then
 * g += momentum buf with nesterov, g = buf without; p -= lr g), 1 = torch.optim.Adam (L2 decay added to the gradient, bias corrections from the chunk's own t),
 * 2 = torch.optim.AdamW (decoupled decay), lr and wd read from hyper.  Then, if ema != NULL, EVERY chunk: e = e d + (1 - d) x, x the value after the update.
 * A chunk that is not active, or of kind 3 / 4, keeps its state, m1, m2 and t.
 * ACH_ERR_INVALID, nothing launched: a NULL state, grad, flags or hyper; chunks or param_chunks < 1, param_chunks > chunks, chunks > 2^30; kind outside 0..2; sgd with
 * momentum != 0 and m1 NULL; adam / adamw with m1, m2 or t NULL, a beta outside [0, 1) or eps < 0; a misaligned pointer. */
int ach_optim_tick(double* hyper, void* stream);
int ach_optim_step(float* state, float* ema, const float* grad, float* m1, float* m2, const int32_t* flags, int32_t* t, const double* hyper, int64_t chunks,
                   int64_t param_chunks, int32_t kind, int32_t nesterov, double momentum, double beta1, double beta2, double eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACHELOUS_OPTIM_H_ */
