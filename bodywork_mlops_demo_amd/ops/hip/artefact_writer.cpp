#include "artefact_writer.h"

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <exception>
#include <stdexcept>

#include <fcntl.h>
#include <unistd.h>

namespace artefact {

std::string npy_header(uint64_t n) {
  const std::string digits = std::to_string(n);
  std::string dict =
      "{'descr': '<f4', 'fortran_order': False, 'shape': (" + digits + ",), }";
  // numpy's spare room for growing axis 0 in place
  constexpr size_t kGrowthDigits = 21;
  if (digits.size() < kGrowthDigits)
    dict.append(kGrowthDigits - digits.size(), ' ');
  // magic(6) + version(2) + uint16 length, then dict + pad + '\n'; numpy
  // always pads by 1..64, never by 0
  constexpr size_t kPrefix = 10, kAlign = 64;
  const size_t hlen = dict.size() + 1;
  const size_t pad = kAlign - ((kPrefix + hlen) % kAlign);
  const size_t total = hlen + pad;  // <= 65535 by a wide margin
  std::string out("\x93NUMPY\x01\x00", 8);
  out.push_back(static_cast<char>(total & 0xff));
  out.push_back(static_cast<char>((total >> 8) & 0xff));
  out += dict;
  out.append(pad, ' ');
  out.push_back('\n');
  return out;
}

bool FileJob::done() const {
  std::lock_guard<std::mutex> lk(mu_);
  return state_ != kPending;
}

FileJob::State FileJob::wait() const {
  std::unique_lock<std::mutex> lk(mu_);
  cv_.wait(lk, [this] { return state_ != kPending; });
  return state_;
}

std::string FileJob::error() const {
  std::lock_guard<std::mutex> lk(mu_);
  return error_;
}

FileJob::Timings FileJob::timings() const {
  std::lock_guard<std::mutex> lk(mu_);
  return timings_;
}

void FileJob::finish(State s, std::string err) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    state_ = s;
    error_ = std::move(err);
  }
  cv_.notify_all();
}

static double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0)
      .count();
}

static std::string errno_text(const char* what, const std::string& path,
                              int err) {
  return std::string(what) + " " + path + ": " + std::strerror(err);
}

void FileJob::run() {
  auto t0 = std::chrono::steady_clock::now();
  if (ready_) {
    try {
      ready_();
    } catch (const std::exception& e) {
      finish(kFailed, std::string("ready: ") + e.what());
      return;
    } catch (...) {
      finish(kFailed, "ready: unknown error");
      return;
    }
  }
  timings_.ready_s = seconds_since(t0);
  t0 = std::chrono::steady_clock::now();
  // same directory as the destination, so the rename stays on one
  // filesystem, and the hidden prefix LocalStore uses for its own
  // temporaries (list_keys skips it)
  const size_t slash = path_.rfind('/');
  std::string tmp = (slash == std::string::npos ? std::string(".")
                                                : path_.substr(0, slash)) +
                    "/.tmp-XXXXXX";
  const int fd = ::mkstemp(&tmp[0]);
  if (fd < 0) {
    finish(kFailed, errno_text("mkstemp", tmp, errno));
    return;
  }
  std::string err;
  const char* p = data_;
  size_t left = size_;
  while (left > 0) {
    const ssize_t w = ::write(fd, p, left);
    if (w < 0) {
      if (errno == EINTR) continue;
      err = errno_text("write", tmp, errno);
      break;
    }
    p += w;
    left -= static_cast<size_t>(w);
  }
  if (::close(fd) != 0 && err.empty()) err = errno_text("close", tmp, errno);
  timings_.write_s = seconds_since(t0);
  t0 = std::chrono::steady_clock::now();
  if (err.empty() && ::rename(tmp.c_str(), path_.c_str()) != 0)
    err = errno_text("rename to", path_, errno);
  if (!err.empty()) {
    ::unlink(tmp.c_str());
    finish(kFailed, std::move(err));
    return;
  }
  timings_.rename_s = seconds_since(t0);
  finish(kDone, "");
}

WriterPool::WriterPool(int workers) {
  if (workers < 1) throw std::invalid_argument("WriterPool needs >= 1 worker");
  threads_.reserve(static_cast<size_t>(workers));
  for (int i = 0; i < workers; ++i)
    threads_.emplace_back([this] { worker_loop(); });
}

WriterPool::~WriterPool() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stopping_ = true;
  }
  cv_.notify_all();
  for (auto& t : threads_)
    if (t.joinable()) t.join();
}

void WriterPool::submit(std::shared_ptr<FileJob> job) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (stopping_) throw std::logic_error("WriterPool is shutting down");
    queue_.push_back(std::move(job));
  }
  cv_.notify_one();
}

void WriterPool::worker_loop() {
  for (;;) {
    std::shared_ptr<FileJob> job;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [this] { return stopping_ || !queue_.empty(); });
      if (queue_.empty()) return;  // stopping and drained
      job = std::move(queue_.front());
      queue_.pop_front();
    }
    job->run();
  }
}

}  // namespace artefact
