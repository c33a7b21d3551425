// host_pool.h -- the process' two worker pools: the per-frame pool (the per-frame half of the fold) and the merge pool (the
// solves of the ordered half).  Host code only; the pools and their mutexes are defined once, in host_abi.cpp.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace g1s {

// Minimal persistent worker pool: the per-frame half of the fold (AR solve,
// block measurements, strength solve) is independent across frames.
class Pool {
 public:
  explicit Pool(unsigned n) {
    for (unsigned i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : workers_) t.join();
  }
  // runs fn(i) for i in [0, n); the caller participates.  Every call has its own job object (function, count, claim and
  // completion counters): a worker that comes late to an earlier job holds THAT job, finds it exhausted and goes back to
  // sleep -- it can never claim an index of a newer job or run the newer function with an older count.
  void parallel_for(int n, const std::function<void(int)> &fn) {
    if (n <= 0) return;
    auto job = std::make_shared<Job>();
    job->fn = &fn;
    job->n = n;
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = job;
      ++epoch_;
    }
    cv_.notify_all();
    work(*job);
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return job->done.load() == job->n; });
    if (job_ == job) job_.reset();
  }

 private:
  struct Job {
    const std::function<void(int)> *fn = nullptr;
    int n = 0;
    std::atomic<int> next{0}, done{0};
  };
  void work(Job &job) {
    int mine = 0;
    for (;;) {
      const int i = job.next.fetch_add(1);
      if (i >= job.n) break;
      (*job.fn)(i);  // (fn outlives the job: parallel_for returns only when done == n)
      ++mine;
    }
    if (mine && job.done.fetch_add(mine) + mine == job.n) {
      std::lock_guard<std::mutex> lk(m_);  // (the waiter checks under this lock: no lost wake-up)
      cv_done_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || epoch_ != seen; });
        if (stop_) return;
        seen = epoch_;
        job = job_;
      }
      if (job) work(*job);
    }
  }
  std::vector<std::thread> workers_;
  std::mutex m_;
  std::condition_variable cv_, cv_done_;
  std::shared_ptr<Job> job_;
  uint64_t epoch_ = 0;
  bool stop_ = false;
};

unsigned usable_cpus();  // the cores this process may really use (the cgroup's quota)
Pool *shared_pool();     // the per-frame pool, nullptr where the process has one thread for it (G1S_FOLD_THREADS)
Pool *merge_pool();      // the merge pool, likewise (G1S_MERGE_POOL)

// fn(i) for i in [0, n) on the per-frame pool / on the merge pool, the calling thread taking part.  parallel_for is not
// re-entrant, so each pool runs one job at a time, under its mutex.  One rule for every caller: a job of one item, and any
// job where the process has no such pool, is a plain loop on the calling thread -- the same result without the lock and
// the hand-over.
void on_shared_pool(int n, const std::function<void(int)> &fn);
void on_merge_pool(int n, const std::function<void(int)> &fn);

}  // namespace g1s
