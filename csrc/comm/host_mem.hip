// Exact-size page-locked host buffers for CPU offload (utils/pinned.py; SURVEY C7, chapter 05).
//
// PyTorch's caching host allocator rounds every pinned block up to a power of two, which the 405B
// offload shards cannot afford.  `pinned_zeros` allocates the requested size (to the page) with
// hipHostMalloc -- memory that is born page-locked, so it needs no registration of pages the
// process already owns (hipHostRegister, which not every host / hypervisor supports) -- and hands
// it out as a zero-filled uint8 tensor.  The tensor's STORAGE owns the allocation: the deleter
// runs when the last view is gone, and hipHostFree drains the device first, so an asynchronous
// copy still reading / writing the pages never sees them freed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include <ATen/ATen.h>
#include <torch/library.h>

namespace dtg {
namespace host_mem {

// Set once the interpreter starts to exit: buffers still alive then are left to the OS, because
// a device drain that late can hang.
std::atomic<bool> g_exiting{false};

at::Tensor pinned_zeros(int64_t nbytes) {
  TORCH_CHECK(nbytes > 0, "pinned_zeros needs a positive size");
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, (size_t)nbytes, hipHostMallocDefault);
  TORCH_CHECK(e == hipSuccess && p != nullptr, "pinned_zeros: hipHostMalloc(", nbytes,
              ") failed: ", hipGetErrorString(e));
  auto t = at::from_blob(p, {nbytes}, [](void* q) {
             if (!g_exiting.load(std::memory_order_relaxed)) (void)hipHostFree(q);
           },
           at::TensorOptions().dtype(at::kByte));
  t.zero_();
  return t;
}

void keep_at_exit() { g_exiting.store(true, std::memory_order_relaxed); }

TORCH_LIBRARY(dtg_host, m) {
  m.def("pinned_zeros(int nbytes) -> Tensor", &pinned_zeros);
  m.def("keep_at_exit() -> ()", &keep_at_exit);
}

}  // namespace host_mem
}  // namespace dtg
