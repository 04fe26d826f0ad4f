// worker_pool.hpp -- the process-wide pool of entropy-decoding workers (worker_pool.cpp).  parallel_for and default_threads are
// for every caller (host_decoder.hpp hands them on); the pool itself, its abort flag and the waits' Backoff are for the host
// decoder's own translation units.
#ifndef MIJ_WORKER_POOL_HPP
#define MIJ_WORKER_POOL_HPP

#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace mij {

int default_threads();

// Run fn(i) for i in [0, n) on the entropy-decoder worker pool (used for large host-side pixel copies).
void parallel_for(int n, const std::function<void(int)> &fn);

// set while a pool thread runs a task: a parallel_for issued from inside one (e.g. the marker search of a stream that
// is itself parsed as one of many in a batch) runs inline instead of waiting for the pool it is part of
extern thread_local bool t_in_pool_worker;

// Waiting for something another pool thread is about to do: a few looks in a row, then naps.  A container's CPU quota (cgroup
// cpu.max) is spent by spinning threads as by working ones, and a process that runs out of it is stopped -- every thread of it --
// until the 100 ms period ends: back-to-back reads of config 5's -rR 4 stream took 21, 21, 52 ms on a box with 16 CPUs' worth
// of quota while the waits were yield loops (profiles/r05/host_refine_times.txt).  The pool threads keep their timer slack at
// a microsecond so that a nap is as long as it says.
// A pool task that died of an exception (out of memory): the tasks that wait for what it would have produced -- the scan
// pipeline's rows -- leave through this instead of waiting for ever; the pool hands the first exception to the caller of wait().
extern std::atomic<bool> g_pool_task_failed;
struct PoolAborted {};
struct Backoff {
  int looks = 0;
  const int spins, nap_us;
  Backoff(int spins_, int nap_us_) : spins(spins_), nap_us(nap_us_) {}
  inline void wait()
  {
    static const bool spin_only = getenv("MIJPEG_SPIN_WAITS") != nullptr; // A-B measurements
    if (t_in_pool_worker && g_pool_task_failed.load(std::memory_order_relaxed)) throw PoolAborted{};
    if (++looks <= spins || spin_only) std::this_thread::yield();
    else std::this_thread::sleep_for(std::chrono::microseconds(nap_us));
  }
};

// Threads are created once (thread creation costs more than decoding a frame on a many-core host) and parked on a condition
// variable between frames.
class WorkerPool {
public:
  static WorkerPool &instance();
  // run fn(i), i in [0, n), on n pool threads; returns immediately, wait() blocks until all returned.
  // false: the threads could not be created (the caller then runs the tasks itself, in order)
  bool start(int n, const std::function<void(int)> &fn);
  void wait();
  // serialises whole frames: one decode uses the pool at a time
  std::mutex frame_mutex;

private:
  WorkerPool() {}
  ~WorkerPool();
  void loop(int id);
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  std::function<void(int)> fn_;
  int want_ = 0, finished_ = 0;
  std::exception_ptr failure_;
  uint64_t generation_ = 0;
  bool stop_ = false;
};

} // namespace mij
#endif
