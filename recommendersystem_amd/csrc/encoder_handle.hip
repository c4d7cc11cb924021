// The shared core of the item-similarity and search handles (encoder_handle.hpp): host code only, the kernels it launches are the
// library's (launch_cast, launch_sumsq, launch_adamw, launch_gemm).
#include <string.h>

#include <cmath>
#include <string>

#include "encoder_handle.hpp"

namespace rsys {

int enc_alloc(EncoderCore* h, void** p, size_t bytes) {
  bytes = std::max<size_t>(256, (bytes + 255) / 256 * 256);
  HIP_CHECK(hipMalloc(p, bytes));
  HIP_CHECK(hipMemset(*p, 0, bytes));
  h->allocs.push_back(*p);
  return RSYS_OK;
}

int enc_check_device(const char* api, int dtype, int device) {
  const std::string who = std::string(api) + "_create: ";
  ARG_CHECK(dtype == RSYS_DTYPE_FP32 || dtype == RSYS_DTYPE_BF16, who + "dtype must be RSYS_DTYPE_FP32 or RSYS_DTYPE_BF16");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error(who + "no HIP device visible"); return RSYS_ERR_HIP; }
  ARG_CHECK(device >= 0 && device < ndev, who + "device index out of range");
  HIP_CHECK(hipSetDevice(device));
  return RSYS_OK;
}

int enc_init(EncoderCore* h, float ls0) {
  h->nflat = h->nw() + 4;
  HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  ENC_ALLOC(h->feat, (size_t)h->fpad * h->fcols * 4);
  ENC_ALLOC(h->P, h->nflat * 4); ENC_ALLOC(h->G, h->nflat * 4); ENC_ALLOC(h->M1, h->nflat * 4); ENC_ALLOC(h->M2, h->nflat * 4);
  if (h->bf16_mode()) ENC_ALLOC(h->Wsh, h->nflat * 2);
  ENC_ALLOC(h->sumsq, 16); ENC_ALLOC(h->sq_part, (size_t)sumsq_parts() * 4);
  HIP_CHECK(hipMemcpy(h->ls(), &ls0, 4, hipMemcpyHostToDevice));   // W stays zero until set
  return RSYS_OK;
}

void enc_free(EncoderCore* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  h->free_own();
  for (void* p : h->allocs) hipFree(p);
  h->slab.release();
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int EncoderCore::features_ready() {
  HIP_CHECK(hipStreamSynchronize(stream));
  has_features = true;
  return RSYS_OK;
}

// name -> (offset, size) in the flat buffers
static int enc_tensor(EncoderCore* h, const char* name, long long* off, long long* size) {
  ARG_CHECK(name, std::string(h->api) + ": null name");
  if (strcmp(name, h->wname) == 0) { *off = 0; *size = h->nw(); return RSYS_OK; }
  if (strcmp(name, "logit_scale") == 0) { *off = h->nw(); *size = 1; return RSYS_OK; }
  set_error(std::string(h->api) + ": unknown parameter '" + name + "' (trainable: " + h->wname + ", logit_scale; the frozen table goes through " +
            h->api + "_features_set)");
  return RSYS_ERR_ARG;
}

int enc_param_io(EncoderCore* h, const char* name, float* out, const float* in, int64_t n, int grad) {
  long long off, size;
  ENC_RC(enc_tensor(h, name, &off, &size));
  ARG_CHECK(n == size, std::string(h->api) + ": element count does not match the parameter's");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  float* base = grad ? h->G : h->P;
  if (out) HIP_CHECK(hipMemcpy(out, base + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (in) {
    HIP_CHECK(hipMemcpy(base + off, in, (size_t)n * 4, hipMemcpyHostToDevice));
    if (h->bf16_mode()) ENC_RC(launch_cast<bf16>(h->P, h->Wsh, h->nw(), h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  return RSYS_OK;
}

int enc_zero_grad(EncoderCore* h) {
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipMemsetAsync(h->G, 0, (size_t)h->nflat * 4, h->stream));
  return RSYS_OK;
}

static int enc_need_adam(EncoderCore* h, const char* call) {
  if (h->has_adam) return RSYS_OK;
  set_error(std::string(h->api) + call + ": no optimizer (" + h->api + "_adamw_create)");
  return RSYS_ERR_STATE;
}

int enc_adamw_step(EncoderCore* h, float lr, float clip, float* norm_out, int32_t* skipped_out) {
  ENC_RC(enc_need_adam(h, "_adamw_step"));
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  ENC_RC(launch_sumsq(h->G, h->nflat, h->sumsq, h->sq_part, s, true));
  float ss = 0.f;
  HIP_CHECK(hipMemcpyAsync(&ss, h->sumsq, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  const float norm = sqrtf(ss);
  const bool skip = !std::isfinite(norm);
  if (norm_out) *norm_out = norm;
  if (skipped_out) *skipped_out = skip ? 1 : 0;
  if (skip) {   // GradScaler: no update and no step count; the gradient is cleared as the next zero_grad would
    HIP_CHECK(hipMemsetAsync(h->G, 0, (size_t)h->nflat * 4, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return RSYS_OK;
  }
  ++h->adam_step;
  if (h->bf16_mode())
    ENC_RC(launch_adamw<bf16>(h->P, h->G, h->M1, h->M2, h->Wsh, h->nw(), h->nflat, lr, h->b1, h->b2, h->eps, h->wd, h->adam_step, h->sumsq, 1.f,
                              clip, 1, s));
  else
    ENC_RC(launch_adamw<float>(h->P, h->G, h->M1, h->M2, (float*)nullptr, h->nw(), h->nflat, lr, h->b1, h->b2, h->eps, h->wd, h->adam_step,
                               h->sumsq, 1.f, clip, 1, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

int enc_adamw_state_io(EncoderCore* h, const char* name, float* m_out, float* v_out, const float* m_in, const float* v_in, int64_t n) {
  ENC_RC(enc_need_adam(h, "_adamw_state"));
  long long off, size;
  ENC_RC(enc_tensor(h, name, &off, &size));
  ARG_CHECK(n == size, std::string(h->api) + "_adamw_state: element count does not match the parameter's");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  if (m_out) HIP_CHECK(hipMemcpy(m_out, h->M1 + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (v_out) HIP_CHECK(hipMemcpy(v_out, h->M2 + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (m_in) HIP_CHECK(hipMemcpy(h->M1 + off, m_in, (size_t)n * 4, hipMemcpyHostToDevice));
  if (v_in) HIP_CHECK(hipMemcpy(h->M2 + off, v_in, (size_t)n * 4, hipMemcpyHostToDevice));
  return RSYS_OK;
}

int enc_features_set(EncoderCore* h, const float* features, int64_t V, int64_t F) {
  const std::string who = std::string(h->api) + "_features_set: ";
  ARG_CHECK(features, who + "null table");
  ARG_CHECK(V == h->frows, who + "the row count must be the handle's item count");
  ARG_CHECK(F == h->fcols, who + "the width must be the handle's feature width");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipMemcpy(h->feat, features, (size_t)V * F * 4, hipMemcpyHostToDevice));
  return h->features_ready();
}

int enc_features_from_device(EncoderCore* h, const float* rows, int64_t V, int64_t F, int device) {
  const std::string who = std::string(h->api) + "_features_from_model: ";
  ARG_CHECK(V == h->frows, who + "the medium's item count must be the handle's");
  ARG_CHECK(F == h->fcols, who + "the model's embed_dim must be the handle's feature width");
  ARG_CHECK(device == h->device, who + "the model and the handle must be on one device");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipMemcpyAsync(h->feat, rows, (size_t)V * F * 4, hipMemcpyDeviceToDevice, h->stream));
  return h->features_ready();
}

template <typename T>
int enc_ordered_gemm(EncoderCore* h, GemmParams p, bool a_km, bool b_km, int* splits_out) {
  ENC_RC(h->slab.reserve(256 * 4, h->stream));
  p.slab = (float*)h->slab.p; p.slab_floats = (long long)(h->slab.bytes / 4);
  ENC_RC(h->slab.reserve((size_t)std::max<long long>(256, gemm_slab_need<T>(p, false, false, a_km, b_km)) * 4, h->stream));
  p.slab = (float*)h->slab.p; p.slab_floats = (long long)(h->slab.bytes / 4);
  if (splits_out) *splits_out = gemm_route<T>(p, false, false, a_km, b_km, cu_count()).splitk;
  return launch_gemm<T>(p, false, false, a_km, b_km, h->stream);
}
template int enc_ordered_gemm<bf16>(EncoderCore*, GemmParams, bool, bool, int*);
template int enc_ordered_gemm<float>(EncoderCore*, GemmParams, bool, bool, int*);

}  // namespace rsys
