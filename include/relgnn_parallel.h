/*
 * relgnn_parallel.h — C ABI of librelgnn.so, data-parallel training (Sparse_Graph_Model.train(group=...), parallel.py).
 *
 * Declared beside relgnn.h, whose conventions hold here too: `stream` is a hipStream_t passed as void*, all work is enqueued
 * asynchronously, every entry point returns an int status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.
 *
 * The step of a rank, between its backward and the one all-reduce(SUM) of the flat gradient buffer:
 *     flat[off_i + j] = s * grad_i[j]        s = float32(w_rank / sum_r w_r), the quotient formed in double on the host
 * for every trainable variable i in optimizer order, off_i = sum of the sizes in front of it.  After the collective the buffer
 * IS the weighted mean gradient: no weight slot rides in it and nothing is divided behind it.
 */
#ifndef RELGNN_PARALLEL_H_
#define RELGNN_PARALLEL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Multi-tensor scaled pack: n <= RELGNN_MT_MAX (relgnn.h) tensors written one behind the other from dst,
 *     dst[off_i + j] = scale * g_i[j],   0 <= j < h_sizes[i],   off_i = h_sizes[0] + ... + h_sizes[i - 1].
 * h_grads and h_sizes are HOST arrays; the device pointers in h_grads travel to the kernel by value in its arguments (no
 * host-to-device copy: the launch can be captured into a hipGraph).  A NULL h_grads[i] writes +0.0f for that tensor's length
 * (a variable that received no gradient; every variable of a rank that takes part in a step without a batch).
 * The product is ONE round-to-nearest fp32 multiply per element: the bits of `g * scale` in torch; 0 * inf and NaN
 * propagate as there.  Sources and dst may start at any 4-byte alignment, independently: 16-byte stores from the first
 * 16-byte boundary of a destination slice on (16-byte loads too where the source then is aligned as well), scalar
 * accesses in front of it and for the last h_sizes[i] % 4 elements.  The result does not depend on the grid or the
 * access width.  Sizes of 0 are legal; exactly sum_i h_sizes[i] floats are written.  A source may not overlap dst.
 * RELGNN_EINVAL: n < 0, n > RELGNN_MT_MAX, a negative size, a NULL table or dst with something to write, a pointer that is not
 * 4-byte aligned. */
int relgnn_mt_pack_scaled_f32(const float* const* h_grads, const int64_t* h_sizes, int32_t n, float scale, float* dst,
                              void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_PARALLEL_H_ */
