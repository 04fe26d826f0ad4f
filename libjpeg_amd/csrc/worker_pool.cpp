// worker_pool.cpp -- the pool of worker_pool.hpp: its threads, parallel_for on top of it and the default worker count.
#if defined(__linux__)
#include <sys/prctl.h>
#endif
#include "worker_pool.hpp"

#include <algorithm>
#include <system_error>

namespace mij {

thread_local bool t_in_pool_worker = false;
std::atomic<bool> g_pool_task_failed{false};

WorkerPool &WorkerPool::instance()
{
  static WorkerPool pool;
  return pool;
}

bool WorkerPool::start(int n, const std::function<void(int)> &fn)
{
  std::unique_lock<std::mutex> lk(mu_);
  try {
    while ((int)threads_.size() < n) {
      const int id = (int)threads_.size();
      threads_.emplace_back([this, id] { loop(id); });
    }
  } catch (const std::system_error &) {
    return false;
  }
  fn_ = fn;
  want_ = n;
  finished_ = 0;
  failure_ = nullptr;
  g_pool_task_failed.store(false);
  generation_++;
  lk.unlock();
  cv_.notify_all();
  return true;
}

void WorkerPool::wait()
{
  std::unique_lock<std::mutex> lk(mu_);
  done_cv_.wait(lk, [this] { return finished_ == want_; });
  if (failure_) { // what a task threw goes to the thread that asked for the work (and from there to the C boundary's handler)
    std::exception_ptr e = failure_;
    failure_ = nullptr;
    g_pool_task_failed.store(false);
    lk.unlock();
    std::rethrow_exception(e);
  }
}

WorkerPool::~WorkerPool()
{
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
    generation_++;
  }
  cv_.notify_all();
  for (auto &t : threads_) t.join();
}

void WorkerPool::loop(int id)
{
#if defined(__linux__)
  prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL); // (nanoseconds; see Backoff)
#endif
  uint64_t seen = 0;
  for (;;) {
    // (no copy of the function object -- a copy allocates, and this thread has nobody to report to: fn_ stands still until every
    // task of the generation has returned, start() only runs behind the previous wait())
    const std::function<void(int)> *fnp = nullptr;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return generation_ != seen; });
      seen = generation_;
      if (stop_) return;
      if (id >= want_) continue;
      fnp = &fn_;
    }
    const std::function<void(int)> &fn = *fnp;
    t_in_pool_worker = true;
    std::exception_ptr thrown;
    try {
      fn(id);
    } catch (const PoolAborted &) { // (left a wait because another task failed: that one's exception is the verdict)
    } catch (...) {
      thrown = std::current_exception();
      g_pool_task_failed.store(true);
    }
    t_in_pool_worker = false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (thrown && !failure_) failure_ = thrown;
      finished_++;
    }
    done_cv_.notify_all();
  }
}

void parallel_for(int n, const std::function<void(int)> &fn)
{
  if (n <= 1 || t_in_pool_worker) {
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  WorkerPool &pool = WorkerPool::instance();
  std::lock_guard<std::mutex> frame(pool.frame_mutex);
  if (!pool.start(n, fn)) {
    // no threads to be had: in order, by the caller (tasks that wait for one another -- the scan pipeline -- only ever wait
    // for tasks with smaller numbers)
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  pool.wait();
}

// Default worker count: every hardware thread up to a cap (MIJPEG_THREADS overrides).  Beyond a few dozen
// workers a single frame has too few restart-interval runs per worker to pay for the wake-ups.
int default_threads()
{
  static const int n = [] {
    if (const char *e = getenv("MIJPEG_THREADS")) {
      const int v = atoi(e);
      if (v > 0) return v;
    }
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (int)std::min(hw, 64u);
  }();
  return n;
}

} // namespace mij
