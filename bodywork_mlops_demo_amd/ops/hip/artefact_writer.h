// Host-side artefact writer: complete file images go from memory to
// <dir>/.tmp-XXXXXX and are renamed into place by a small pool of
// std::threads.  Plain C++17 (no HIP, no torch, no Python) so it also
// compiles stand-alone for the host sanitizer test
// (tests/asan/artefact_writer_host.cpp).
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace artefact {

// The exact bytes np.save writes in front of a 1-D little-endian float32
// array of n elements (format 1.0): magic, uint16 length, then the dict
// {'descr': '<f4', 'fortran_order': False, 'shape': (n,), } space-padded
// and newline-terminated so the whole header is a multiple of 64 bytes.
// Like numpy >= 1.25 the dict is first padded as if n had 21 digits, so
// an array can grow in place.
std::string npy_header(uint64_t n);

// One file to write.  `data` must stay valid and unchanged until the job
// has left the pending state; the pool keeps no other reference to it.
class FileJob {
 public:
  enum State { kPending, kDone, kFailed };

  FileJob(std::string path, const void* data, size_t size,
          std::function<void()> ready = nullptr)
      : path_(std::move(path)), data_(static_cast<const char*>(data)),
        size_(size), ready_(std::move(ready)) {}

  bool done() const;          // true once done OR failed
  State wait() const;         // blocks until the job left kPending
  std::string error() const;  // strerror-style text when failed, else ""
  const std::string& path() const { return path_; }

  // seconds the worker spent per step; valid once done() is true
  struct Timings { double ready_s = 0, write_s = 0, rename_s = 0; };
  Timings timings() const;

 private:
  friend class WriterPool;
  void run();                  // on a worker thread
  void finish(State s, std::string err);

  const std::string path_;
  const char* const data_;
  const size_t size_;
  // called on the worker before anything is opened (e.g. waits for the
  // copy that fills `data`); an exception it throws fails the job
  std::function<void()> ready_;

  mutable std::mutex mu_;
  mutable std::condition_variable cv_;
  State state_ = kPending;
  std::string error_;
  Timings timings_;  // written by the worker before finish()
};

// W workers taking FileJobs from a FIFO queue.  A failed job never takes
// the pool down.  The destructor lets the workers finish every queued job
// and joins them.
class WriterPool {
 public:
  explicit WriterPool(int workers);
  ~WriterPool();
  WriterPool(const WriterPool&) = delete;
  WriterPool& operator=(const WriterPool&) = delete;

  void submit(std::shared_ptr<FileJob> job);
  int workers() const { return static_cast<int>(threads_.size()); }

 private:
  void worker_loop();

  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<FileJob>> queue_;
  bool stopping_ = false;
  std::vector<std::thread> threads_;
};

}  // namespace artefact
