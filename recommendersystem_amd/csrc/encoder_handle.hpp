// What the handles that are independent of rsys_model share (similarity.hip: rsys_sim_*, search.hip: rsys_search_*): a stream of their
// own, a frozen fp32 feature table, one trainable matrix W and a scalar logit_scale in a flat buffer [W | logit_scale | 3 pad] with
// matching gradient and AdamW moment buffers, a bf16 shadow of W, and an fp32 slab for split-K sums in a fixed order.  A model embeds
// the core by inheriting from it and keeps what is its own: kernels, per-call buffers, forward / backward, export and serving calls.
// The grow-on-demand device buffer and the workspace carver come from workspace.hpp (through model.hpp).
#pragma once
#include <algorithm>
#include <vector>

#include "model.hpp"

namespace rsys {

#define ENC_RC(expr) do { int _rc = (expr); if (_rc != RSYS_OK) return _rc; } while (0)

// `Type* h` of a C entry point's void* handle
#define ENC_HANDLE(Type, hv)                                                    \
  Type* h = static_cast<Type*>((EncoderCore*)(hv));                             \
  do {                                                                          \
    if (h == nullptr) { set_error("null handle"); return RSYS_ERR_ARG; }        \
  } while (0)

inline unsigned grid_for(long long work, int per_block = 256, long long cap = 8192) {
  return (unsigned)std::max<long long>(1, std::min<long long>((work + per_block - 1) / per_block, cap));
}

struct EncoderCore {
  const char* api = "";                             // "rsys_sim" / "rsys_search": which model's call failed
  const char* wname = "";                           // state-dict name of W
  int device = 0, dtype = 0;
  hipStream_t stream = nullptr;
  long long frows = 0, fpad = 0;                    // feature rows, rows allocated (the rest stays zero)
  int fcols = 0, wrows = 0, wcols = 0;              // feat [fpad][fcols], W [wrows][wcols]
  long long nflat = 0;                              // [W | logit_scale | 3 pad]
  float *feat = nullptr, *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr;
  bf16* Wsh = nullptr;                              // bf16 copy of W (bf16 mode)
  float *sumsq = nullptr, *sq_part = nullptr;
  DevScratch slab;                                  // ordered split-K partial tiles
  float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, wd = 0.1f;
  int adam_step = 0;
  bool has_adam = false, has_features = false;
  std::vector<void*> allocs;                        // enc_alloc's pointers, freed by enc_free
  bool bf16_mode() const { return dtype == RSYS_DTYPE_BF16; }
  long long nw() const { return (long long)wrows * wcols; }
  float* ls() const { return P + nw(); }
  virtual ~EncoderCore() {}
  virtual void free_own() {}                        // the model's buffers outside allocs (the stream is idle)
  virtual int features_ready();                     // feat changed: operand copies of it, then the stream idle and has_features set
};

// zeroed device memory, a multiple of 256 bytes, freed with the handle
int enc_alloc(EncoderCore* h, void** p, size_t bytes);
#define ENC_ALLOC(ptr, bytes) ENC_RC(enc_alloc(h, (void**)&(ptr), (size_t)(bytes)))

// dtype and device checks of a create call, before the handle exists; the device is current on return
int enc_check_device(const char* api, int dtype, int device);
// the stream and the common buffers of a new handle (api, wname, device, dtype and the shapes set); logit_scale = ls0
int enc_init(EncoderCore* h, float ls0);
void enc_free(EncoderCore* h);   // waits, h->free_own(), frees what the core holds, deletes h; null: nothing

// out: read, in: write `name` (wname or "logit_scale") of P (grad = 0) or G; a write of P refreshes the bf16 copy
int enc_param_io(EncoderCore* h, const char* name, float* out, const float* in, int64_t n, int grad);
int enc_zero_grad(EncoderCore* h);
// clip by the global norm, AdamW with the handle's hyper-parameters; a non-finite norm skips the update and clears G (GradScaler).
// RSYS_ERR_STATE without an optimizer.
int enc_adamw_step(EncoderCore* h, float lr, float clip, float* norm_out, int32_t* skipped_out);
int enc_adamw_state_io(EncoderCore* h, const char* name, float* m_out, float* v_out, const float* m_in, const float* v_in, int64_t n);
int enc_features_set(EncoderCore* h, const float* features, int64_t V, int64_t F);                        // from the host
int enc_features_from_device(EncoderCore* h, const float* rows, int64_t V, int64_t F, int device);        // from a model's table

// A product whose sum must have a fixed order (EPI_ATOMIC into fp32 C): with a slab in its parameters launch_gemm stays off the
// split-K forms that add partial tiles with float atomics (gemm8p's mixed-layout form, gemm4k), and every K split stores its partial
// tile into the slab, summed in split order afterwards.  The slab is present when the need is asked, as it is at the launch, so
// the size is the routed kernel's.  splits_out (may be null): the K splits the launch runs with, from the route launch_gemm reads.
template <typename T>
int enc_ordered_gemm(EncoderCore* h, GemmParams p, bool a_km, bool b_km, int* splits_out = nullptr);

}  // namespace rsys
