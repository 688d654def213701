// Stand-alone host driver for ops/hip/artefact_writer.* (built by
// tests/test_artefact_writer_cpu.py under ASAN+UBSAN and under TSAN):
// 16 jobs of 1 B .. 1 MiB through a 3-worker pool with 4 reused buffers,
// one of them into a directory that does not exist, then a pool that is
// destroyed with jobs still queued.  Exit 0 = every check held.
#include <dirent.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../bodywork_mlops_demo_amd/ops/hip/artefact_writer.h"

using artefact::FileJob;
using artefact::WriterPool;

static int failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      ++failures;                                     \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);              \
      std::fprintf(stderr, "\n");                     \
    }                                                 \
  } while (0)

// byte k of job i's image
static char image_byte(int job, size_t k) {
  return static_cast<char>((k * 131u + static_cast<size_t>(job) * 17u + 7u) &
                           0xff);
}

static void fill(char* buf, int job, size_t n) {
  for (size_t k = 0; k < n; ++k) buf[k] = image_byte(job, k);
}

static bool file_holds(const std::string& path, int job, size_t n) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::vector<char> got((std::istreambuf_iterator<char>(f)),
                        std::istreambuf_iterator<char>());
  if (got.size() != n) return false;
  for (size_t k = 0; k < n; ++k)
    if (got[k] != image_byte(job, k)) return false;
  return true;
}

static int count_tmp(const std::string& dir) {
  int n = 0;
  DIR* d = opendir(dir.c_str());
  if (!d) return -1;
  while (dirent* e = readdir(d))
    if (std::strncmp(e->d_name, ".tmp-", 5) == 0) ++n;
  closedir(d);
  return n;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <existing empty directory>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];

  // header shape: magic, little-endian length, 64-byte multiple, newline
  for (uint64_t n : {0ull, 1ull, 999ull, 1000000000000ull}) {
    const std::string h = artefact::npy_header(n);
    CHECK(h.size() % 64 == 0 && h.size() >= 64, "header size %zu", h.size());
    CHECK(h.compare(0, 8, std::string("\x93NUMPY\x01\x00", 8)) == 0, "magic");
    const size_t len = static_cast<unsigned char>(h[8]) |
                       (static_cast<size_t>(static_cast<unsigned char>(h[9]))
                        << 8);
    CHECK(len + 10 == h.size(), "length field %zu vs %zu", len, h.size());
    CHECK(h.back() == '\n', "header must end in a newline");
    CHECK(h.find("'shape': (" + std::to_string(n) + ",), }") !=
              std::string::npos, "shape of %llu missing",
          static_cast<unsigned long long>(n));
  }

  const size_t kMiB = 1u << 20;
  const size_t sizes[16] = {1,     2,      3,      63,     64,      65,
                            4095,  4096,   4097,   65535,  65536,   100003,
                            262144, 524289, kMiB - 1, kMiB};
  const int kBad = 5;  // destination directory does not exist
  const int kBuffers = 4;
  std::vector<std::vector<char>> bufs(kBuffers, std::vector<char>(kMiB));
  std::vector<std::shared_ptr<FileJob>> jobs(16);
  std::atomic<int> ready_calls{0};
  {
    WriterPool pool(3);
    CHECK(pool.workers() == 3, "workers %d", pool.workers());
    for (int i = 0; i < 16; ++i) {
      const int b = i % kBuffers;
      // a buffer is refilled only after the job that last used it ended
      if (i >= kBuffers) jobs[i - kBuffers]->wait();
      fill(bufs[b].data(), i, sizes[i]);
      const std::string path =
          (i == kBad ? dir + "/no-such-dir" : dir) + "/job-" +
          std::to_string(i) + ".bin";
      jobs[i] = std::make_shared<FileJob>(
          path, bufs[b].data(), sizes[i], [&ready_calls, i] {
            if (i % 3 == 0)
              std::this_thread::sleep_for(std::chrono::milliseconds(2));
            ready_calls.fetch_add(1);
          });
      pool.submit(jobs[i]);
      // the image must be on disk before its buffer is reused, so check
      // jobs as they retire (the last four are checked after the loop)
      if (i >= kBuffers) {
        const int j = i - kBuffers;
        if (j == kBad) continue;
        CHECK(jobs[j]->wait() == FileJob::kDone, "job %d: %s", j,
              jobs[j]->error().c_str());
      }
    }
    for (int i = 0; i < 16; ++i) {
      const FileJob::State st = jobs[i]->wait();
      CHECK(jobs[i]->done(), "job %d not done after wait", i);
      if (i == kBad) {
        CHECK(st == FileJob::kFailed, "bad job must fail");
        CHECK(!jobs[i]->error().empty(), "bad job must carry a message");
        continue;
      }
      CHECK(st == FileJob::kDone, "job %d: %s", i, jobs[i]->error().c_str());
      CHECK(jobs[i]->error().empty(), "job %d has an error text", i);
      CHECK(file_holds(jobs[i]->path(), i, sizes[i]),
            "job %d: file does not hold its image", i);
      const auto t = jobs[i]->timings();
      CHECK(t.ready_s >= 0 && t.write_s >= 0 && t.rename_s >= 0,
            "job %d: negative timing", i);
    }
    CHECK(ready_calls.load() == 16, "ready ran %d times", ready_calls.load());
    CHECK(count_tmp(dir) == 0, "%d temporaries left", count_tmp(dir));
  }

  // a pool destroyed with jobs still queued finishes them and joins
  const int kQueued = 6;
  std::vector<std::vector<char>> qbufs(kQueued, std::vector<char>(4096));
  std::vector<std::shared_ptr<FileJob>> qjobs(kQueued);
  std::atomic<bool> go{false};
  {
    WriterPool pool(1);
    for (int i = 0; i < kQueued; ++i) {
      fill(qbufs[i].data(), 100 + i, qbufs[i].size());
      qjobs[i] = std::make_shared<FileJob>(
          dir + "/queued-" + std::to_string(i) + ".bin", qbufs[i].data(),
          qbufs[i].size(), [&go] {
            // the one worker is held at the first job until the pool is
            // about to be destroyed, so the others are certainly queued
            while (!go.load())
              std::this_thread::sleep_for(std::chrono::milliseconds(1));
          });
      pool.submit(qjobs[i]);
    }
    for (int i = 0; i < kQueued; ++i)
      CHECK(!qjobs[i]->done(), "queued job %d ended before destruction", i);
    go.store(true);
  }
  for (int i = 0; i < kQueued; ++i) {
    CHECK(qjobs[i]->done() && qjobs[i]->wait() == FileJob::kDone,
          "queued job %d: %s", i, qjobs[i]->error().c_str());
    CHECK(file_holds(qjobs[i]->path(), 100 + i, qbufs[i].size()),
          "queued job %d: file does not hold its image", i);
  }
  CHECK(count_tmp(dir) == 0, "%d temporaries left", count_tmp(dir));

  if (failures) return 1;
  std::puts("ok");
  return 0;
}
