// spz_photo_internal.hpp — what spz_refine.hip uses of spz_photo.hip beyond the C ABI: the photo loss with the exposure
// in device memory, and the Adam step of one view's exposure, so that a loop that fits exposures never waits for the
// host.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spz_amd_detail {

// spz_amd_photo_loss_device with the 12 exposure values read from device memory by the kernels (d_exposure NULL: the
// identity, nothing multiplied).  Arguments are the caller's to check.
int photo_loss_enqueue(const float *d_a, int channels_a, const float *d_b, int channels_b, const float *d_weight,
                       const double *d_exposure, int width, int height, double lambda, double *d_loss, float *d_grad,
                       double *d_exposure_grad, void *d_workspace, hipStream_t st);

// One Adam step in f64 over 12 values, one workgroup (torch's form, as "adam step" words it, every operation an f64
// one): m' = beta1 m + (1 - beta1) g;  v' = beta2 v + ((1 - beta2) g) g;  den = sqrt(v') / sqrt(1 - beta2^t) + eps;
// e' = e - (lr / (1 - beta1^t)) (m' / den).  A value whose gradient is not finite is left alone, moments included.
// The scalars of step t are formed on the host in f64.
int photo_exposure_adam_enqueue(double *d_exposure, const double *d_grad, double *d_m, double *d_v, int t, double lr,
                                double beta1, double beta2, double eps, hipStream_t st);

}  // namespace spz_amd_detail
