// sol_stage.h -- the staged host route of the bake families (lightmaps, volumes, depth moments): the caller's arrays copied into ONE
// scratch buffer of the handle (SolScene::lm_stage or vol_stage), the family's device route run over the copies, the outputs copied back. A route
// declares each array once - host pointer, bytes, direction -, calls upload(), hands st[array] to its launch and returns finish(). The layout is the
// declaration order, each array rounded up to 256 bytes; an absent optional array takes none. Nothing here allocates: the capacity is fixed, and
// the buffer only grows (DevBuf::reserve).
#pragma once
#include "sol_scene.h"

class SolStaged {
 public:
  static constexpr int MAX_ARRAYS = 12;  // (the longest route, sol_lightmap_sample_lod, stages eleven)
  SolStaged(hipStream_t stream, DevBuf<char>& buf) : stream_(stream), buf_(buf) {}
  // The declarations return the array's number for operator[]. What the launch gets differs, and launches and kernels branch on null pointers:
  //   in      a required input: always an address, also for 0 bytes (an empty table, no triangles) - those are not copied
  //   in_opt  an optional input: null `host` takes no room and is null at the launch; otherwise as `in`
  //   out     an output: always room and an address; copied back unless `host` is null (the caller did not ask, the launch writes it anyway)
  //   out_opt an optional output: null `host` takes no room and is null at the launch; otherwise as `out`
  int in(const void* host, size_t bytes) { return add(host, nullptr, bytes, true); }
  int in_opt(const void* host, size_t bytes) { return add(host, nullptr, host ? bytes : 0, host != nullptr); }
  int out(void* host, size_t bytes) { return add(nullptr, host, bytes, true); }
  int out_opt(void* host, size_t bytes) { return add(nullptr, host, host ? bytes : 0, host != nullptr); }
  size_t total() const { return total_; }
  size_t offset(int i) const { return a_[i].at; }
  // Room for every array in the buffer, then the inputs copied in on the stream. A failure returns at once.
  int upload() {
    if (full_) return sol_fail(SOL_EINVAL, "SolStaged: more than %d arrays", MAX_ARRAYS);
    if (const int rc = buf_.reserve(stream_, total_)) return rc;
    for (int i = 0; i < n_; ++i)
      if (a_[i].src && a_[i].bytes) HIP_TRY(hipMemcpyAsync(buf_.get() + a_[i].at, a_[i].src, a_[i].bytes, hipMemcpyHostToDevice, stream_));
    return SOL_OK;
  }
  // The device address of array i (after upload), or null where it is absent.
  char* operator[](int i) const { return a_[i].present ? buf_.get() + a_[i].at : nullptr; }
  // The outputs copied back, then the stream drained: the caller's arrays are complete afterwards. (A launch error returns before this is called.)
  int finish() {
    for (int i = 0; i < n_; ++i)
      if (a_[i].dst && a_[i].bytes) HIP_TRY(hipMemcpyAsync(a_[i].dst, buf_.get() + a_[i].at, a_[i].bytes, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(hipStreamSynchronize(stream_));
    return SOL_OK;
  }

 private:
  struct Array { const void* src; void* dst; size_t bytes, at; bool present; };
  int add(const void* src, void* dst, size_t bytes, bool present) {
    if (n_ == MAX_ARRAYS) return full_ = true, 0;  // (upload refuses)
    a_[n_] = {src, dst, bytes, total_, present};
    total_ += (bytes + 255) / 256 * 256;
    return n_++;
  }
  hipStream_t stream_;
  DevBuf<char>& buf_;
  Array a_[MAX_ARRAYS] = {};
  int n_ = 0;
  bool full_ = false;
  size_t total_ = 0;
};
