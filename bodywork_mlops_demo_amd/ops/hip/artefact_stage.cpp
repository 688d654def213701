// Dataset persist without Python between the device copy and the rename.
//
// DatasetPersister stages a day's (y, X) as one complete .npy-pair file
// image in pinned host memory -- [header(n) | y | header(n) | X] -- with
// two D2H copies on a side stream, and hands the image to a WriterPool
// worker that waits for the copy event, writes a temporary file and
// renames it.  The workers never take the GIL, so the stage code on the
// main thread and the file writes do not queue behind each other.  No
// device kernels here, and nothing touches the compute stream beyond one
// event record.
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>

#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "artefact_writer.h"

namespace py = pybind11;

namespace {

inline void hip_check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "DatasetPersister: ", what, ": ",
              hipGetErrorString(e));
}

// what submit() returns: the file job plus how long submit waited for its
// slot's previous write
struct PersistHandle {
  std::shared_ptr<artefact::FileJob> job;
  double slot_wait_s = 0.0;

  bool done() const { return job->done(); }
  void result() const {  // GIL released by the binding
    if (job->wait() == artefact::FileJob::kFailed)
      throw std::runtime_error("dataset persist failed: " + job->error());
  }
  py::dict timings() const {
    const auto t = job->timings();
    py::dict d;
    d["slot_wait_s"] = slot_wait_s;
    d["ready_s"] = t.ready_s;
    d["write_s"] = t.write_s;
    d["rename_s"] = t.rename_s;
    return d;
  }
};

class DatasetPersister {
 public:
  DatasetPersister(int workers, int slots)
      : slots_(static_cast<size_t>(slots)) {
    TORCH_CHECK(workers >= 1 && workers <= 16,
                "DatasetPersister: workers must be in [1, 16]");
    TORCH_CHECK(slots >= 1 && slots <= 64,
                "DatasetPersister: slots must be in [1, 64]");
    pool_ = std::make_unique<artefact::WriterPool>(workers);
  }

  ~DatasetPersister() { close(); }

  // Finish every queued write, join the workers and free the staging
  // memory.  Never throws; a write error that nobody collected is lost.
  void close() noexcept {
    std::lock_guard<std::mutex> lk(mu_);
    pool_.reset();  // drains the queue, joins every worker
    for (auto& s : slots_) {
      s.job.reset();
      if (s.event) (void)hipEventDestroy(s.event);
      if (s.buf) (void)hipHostFree(s.buf);
      s = Slot{};
    }
    if (fork_event_) (void)hipEventDestroy(fork_event_);
    fork_event_ = nullptr;
  }

  PersistHandle submit(const at::Tensor& y, const at::Tensor& X,
                       const std::string& final_path) {
    TORCH_CHECK(y.is_cuda() && X.is_cuda() && y.device() == X.device(),
                "DatasetPersister.submit: y and X must be on one GPU");
    TORCH_CHECK(y.scalar_type() == at::kFloat && X.scalar_type() == at::kFloat
                    && y.dim() == 1 && X.dim() == 1,
                "DatasetPersister.submit: y and X must be 1-D float32");
    TORCH_CHECK(y.is_contiguous() && X.is_contiguous(),
                "DatasetPersister.submit: y and X must be contiguous");
    std::unique_lock<std::mutex> lk(mu_, std::defer_lock);
    {
      // never hold the GIL while waiting for the lock: its holder may be
      // about to take the GIL back
      py::gil_scoped_release nogil;
      lk.lock();
    }
    TORCH_CHECK(pool_ != nullptr, "DatasetPersister is closed");
    if (device_ < 0) device_ = y.get_device();
    TORCH_CHECK(y.get_device() == device_,
                "DatasetPersister.submit: one persister serves one device");
    c10::DeviceGuard guard(y.device());

    Slot& s = slots_[next_];
    PersistHandle h;
    if (s.job) {
      // the slot's image is free once the write that last used it ended
      const auto t0 = std::chrono::steady_clock::now();
      artefact::FileJob::State st;
      {
        py::gil_scoped_release nogil;
        st = s.job->wait();
      }
      h.slot_wait_s = std::chrono::duration<double>(
                          std::chrono::steady_clock::now() - t0).count();
      auto prev = std::move(s.job);
      s.job.reset();
      if (st == artefact::FileJob::kFailed)
        throw std::runtime_error("dataset persist of " + prev->path() +
                                 " failed: " + prev->error());
    }

    const std::string hy = artefact::npy_header(
        static_cast<uint64_t>(y.numel()));
    const std::string hX = artefact::npy_header(
        static_cast<uint64_t>(X.numel()));
    const size_t by = static_cast<size_t>(y.numel()) * sizeof(float);
    const size_t bX = static_cast<size_t>(X.numel()) * sizeof(float);
    const size_t total = hy.size() + by + hX.size() + bX;
    if (s.capacity < total) {
      if (s.buf) hip_check(hipHostFree(s.buf), "hipHostFree");
      s.buf = nullptr;
      s.capacity = 0;
      // day sizes wander by a few thousand rows: leave headroom so a
      // slot is not reallocated for every slightly larger day
      const size_t cap = total + total / 8 + 4096;
      void* p = nullptr;
      hip_check(hipHostMalloc(&p, cap, hipHostMallocDefault),
                "hipHostMalloc");
      s.buf = static_cast<char*>(p);
      s.capacity = cap;
    }
    if (!s.event)
      hip_check(hipEventCreateWithFlags(&s.event, hipEventDisableTiming),
                "hipEventCreate");
    if (!fork_event_)
      hip_check(hipEventCreateWithFlags(&fork_event_, hipEventDisableTiming),
                "hipEventCreate");
    if (!side_) side_ = c10::hip::getStreamFromPoolMasqueradingAsCUDA(false, device_);

    char* at_y = s.buf + hy.size();
    char* at_hX = at_y + by;
    char* at_X = at_hX + hX.size();
    std::memcpy(s.buf, hy.data(), hy.size());
    std::memcpy(at_hX, hX.data(), hX.size());

    // side stream waits for whatever produced y and X on the current
    // stream; the copies land at their offsets in the file image
    const hipStream_t cur = c10::hip::getCurrentHIPStream(device_).stream();
    const hipStream_t side = side_->stream();
    hip_check(hipEventRecord(fork_event_, cur), "hipEventRecord");
    hip_check(hipStreamWaitEvent(side, fork_event_, 0), "hipStreamWaitEvent");
    if (by)
      hip_check(hipMemcpyAsync(at_y, y.data_ptr<float>(), by,
                               hipMemcpyDeviceToHost, side),
                "hipMemcpyAsync(y)");
    if (bX)
      hip_check(hipMemcpyAsync(at_X, X.data_ptr<float>(), bX,
                               hipMemcpyDeviceToHost, side),
                "hipMemcpyAsync(X)");
    hip_check(hipEventRecord(s.event, side), "hipEventRecord");
    // the sources are consumed on the side stream: tell the caching
    // allocator, or their blocks could be handed to a later allocation on
    // the compute stream while the copy is still in flight.  No worker
    // keeps a tensor reference.
    c10::hip::HIPCachingAllocator::recordStream(y.storage().data_ptr(),
                                                side_->hip_stream());
    c10::hip::HIPCachingAllocator::recordStream(X.storage().data_ptr(),
                                                side_->hip_stream());

    const hipEvent_t ev = s.event;
    s.job = std::make_shared<artefact::FileJob>(
        final_path, s.buf, total, [ev] {
          const hipError_t e = hipEventSynchronize(ev);
          if (e != hipSuccess)
            throw std::runtime_error(std::string("hipEventSynchronize: ") +
                                     hipGetErrorString(e));
        });
    pool_->submit(s.job);
    h.job = s.job;
    next_ = (next_ + 1) % slots_.size();
    return h;
  }

  // Wait for every job in flight (GIL released) and raise the first
  // error nobody has seen yet.
  void drain() {
    std::unique_lock<std::mutex> lk(mu_, std::defer_lock);
    std::string first;
    {
      py::gil_scoped_release nogil;
      lk.lock();
      // oldest first: the slot after the newest one
      for (size_t i = 0; i < slots_.size(); ++i) {
        Slot& s = slots_[(next_ + i) % slots_.size()];
        if (!s.job) continue;
        if (s.job->wait() == artefact::FileJob::kFailed && first.empty())
          first = "dataset persist of " + s.job->path() +
                  " failed: " + s.job->error();
        s.job.reset();
      }
    }
    if (!first.empty()) throw std::runtime_error(first);
  }

  int workers() const { return pool_ ? pool_->workers() : 0; }
  int slots() const { return static_cast<int>(slots_.size()); }

 private:
  struct Slot {
    char* buf = nullptr;
    size_t capacity = 0;
    hipEvent_t event = nullptr;
    std::shared_ptr<artefact::FileJob> job;  // last write from this slot
  };

  std::mutex mu_;
  std::vector<Slot> slots_;
  size_t next_ = 0;
  int device_ = -1;
  // non-blocking stream from torch's pool (it outlives every tensor the
  // allocator may still tie to it)
  c10::optional<c10::hip::HIPStreamMasqueradingAsCUDA> side_;
  hipEvent_t fork_event_ = nullptr;
  std::unique_ptr<artefact::WriterPool> pool_;
};

}  // namespace

void bind_artefact_stage(py::module_& m) {
  m.def("npy_header",
        [](uint64_t n) { return py::bytes(artefact::npy_header(n)); },
        "np.save's header bytes for a 1-D float32 array of n elements");
  py::class_<PersistHandle>(m, "PersistHandle")
      .def("done", &PersistHandle::done)
      .def("result", &PersistHandle::result,
           py::call_guard<py::gil_scoped_release>())
      .def("timings", &PersistHandle::timings);
  py::class_<DatasetPersister>(m, "DatasetPersister")
      .def(py::init<int, int>(), py::arg("workers"), py::arg("slots"))
      .def("submit", &DatasetPersister::submit, py::arg("y"), py::arg("X"),
           py::arg("final_path"))
      .def("drain", &DatasetPersister::drain)
      .def("close", &DatasetPersister::close,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("workers", &DatasetPersister::workers)
      .def_property_readonly("slots", &DatasetPersister::slots);
}
