// wg_host.h -- a workgroup on the host, for tests: `threads` logical threads run a callable f(tid, sync) whose `sync` is a
// real barrier, so a function written for a GPU workgroup (one that takes its thread index and its barrier as arguments,
// such as dn_tile of grav1synth_amd/csrc/denoise_tile.hip.h) runs here unmodified.
//
// Serialised (the default).  Every thread is a fibre with a stack of its own.  Between two barriers the fibres run ONE AT A
// TIME, each from the barrier it waits at to its next barrier (or its return), in an order the test chooses for that
// interval: a Schedule, named and seeded.  A workgroup on a device runs its waves close to lockstep; here a thread may be
// a whole phase ahead of its neighbour or behind it, so a phase that reads what another thread has not yet written in
// this interval -- a barrier missing or misplaced -- reads the old bytes and shows in the result.  The fibres are
// announced to AddressSanitizer (__sanitizer_start_switch_fiber / __sanitizer_finish_switch_fiber), so the program is built
// and run with it; older runtimes still print one line of warning when swapcontext is first called.
//
// Free-running (-DWG_FREE_RUNNING).  Every thread is a std::thread and `sync` a plain counting barrier: nothing is
// serialised and the schedule is not used.  This is the form ThreadSanitizer watches.
//
// Barrier divergence -- a thread that returns while others wait at a barrier, which includes threads whose numbers of
// barriers differ -- would hang a device.  Here it is a message on stderr and exit status kDivergence.
//
// skip >= 0 makes the skip-th sync() call (counted from 0) of EVERY thread return at once, without a barrier: the
// experiment "this barrier is not there".  It is the same call in every thread, so the counts still match.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#if defined(WG_FREE_RUNNING)
#include <condition_variable>
#include <mutex>
#include <thread>
#else
#include <sys/mman.h>
#include <ucontext.h>
#if defined(__SANITIZE_ADDRESS__)
#define WG_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define WG_ASAN 1
#endif
#endif
#if defined(WG_ASAN)
#include <sanitizer/common_interface_defs.h>
#endif
#endif

namespace wg {

constexpr int kDivergence = 3;  // exit status of a run whose threads disagree about a barrier
constexpr int kWave = 64;

// splitmix64: the same numbers on every host and with every standard library
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
  void shuffle(std::vector<int> &v) {
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[below((uint32_t)i)]);
  }
};

// the order in which the threads run in one interval between two barriers
struct Schedule {
  enum Kind { kAscending, kDescending, kWavesReversed, kRandom, kStragglers } kind;
  uint64_t seed;
  std::vector<int> late;  // kStragglers: the quarter that always runs last

  static const char *const *names() {
    static const char *const n[] = {"ascending", "descending", "waves-reversed", "random", "stragglers", nullptr};
    return n;
  }
  static bool parse(const char *name, uint64_t seed, Schedule &s) {
    for (int k = 0; names()[k]; ++k)
      if (!std::strcmp(name, names()[k])) return s.kind = (Kind)k, s.seed = seed, true;
    return false;
  }
  // ascending:       tid 0, 1, 2, ...
  // descending:      tid n - 1, n - 2, ...
  // waves-reversed:  the last wave of 64 first, lanes ascending inside a wave
  // random:          a fresh permutation for every interval, from (seed, interval)
  // stragglers:      a quarter of the threads, drawn once from the seed, runs after all the others in every interval
  //                  (both groups ascending)
  void order(int threads, uint64_t interval, std::vector<int> &o) {
    o.resize((size_t)threads);
    switch (kind) {
      case kAscending:
        for (int i = 0; i < threads; ++i) o[i] = i;
        break;
      case kDescending:
        for (int i = 0; i < threads; ++i) o[i] = threads - 1 - i;
        break;
      case kWavesReversed: {
        const int waves = (threads + kWave - 1) / kWave;
        int n = 0;
        for (int w = waves - 1; w >= 0; --w)
          for (int l = w * kWave; l < threads && l < (w + 1) * kWave; ++l) o[n++] = l;
        break;
      }
      case kRandom: {
        for (int i = 0; i < threads; ++i) o[i] = i;
        Rng r(seed * 0x100000001B3ull + interval);
        r.shuffle(o);
        break;
      }
      case kStragglers: {
        if ((int)late.size() != threads) {
          std::vector<int> p((size_t)threads);
          for (int i = 0; i < threads; ++i) p[i] = i;
          Rng r(seed ^ 0x5742u);
          r.shuffle(p);
          late.assign((size_t)threads, 0);
          for (int i = 0; i < threads / 4; ++i) late[p[i]] = 1;
        }
        int n = 0;
        for (int pass = 0; pass < 2; ++pass)
          for (int i = 0; i < threads; ++i)
            if (late[i] == pass) o[n++] = i;
        break;
      }
    }
  }
};

[[noreturn]] inline void diverged(int done_tid, long done_syncs, int wait_tid, long wait_syncs) {
  std::fprintf(stderr,
               "wg: barrier divergence: thread %d returned after %ld sync() calls while thread %d waits in its sync() call number %ld\n",
               done_tid, done_syncs, wait_tid, wait_syncs);
  std::fflush(stderr);
  std::_Exit(kDivergence);
}

struct Stats {
  long syncs = 0;      // sync() calls of each thread (the same for all, or the run has ended with kDivergence)
  long intervals = 0;  // serialised: intervals run
};

#if !defined(WG_FREE_RUNNING)

class Workgroup;
struct Sync {
  Workgroup *wg;
  int tid;
  void operator()() const;
};

class Workgroup {
 public:
  static constexpr size_t kStack = 256 << 10, kGuard = 4096;

  explicit Workgroup(int threads) : n_(threads), f_((size_t)threads) {
    for (auto &f : f_) {
      void *m = mmap(nullptr, kStack + kGuard, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_STACK, -1, 0);
      if (m == MAP_FAILED || mprotect(m, kGuard, PROT_NONE) != 0) std::perror("wg: fibre stack"), std::exit(2);
      f.map = m, f.stack = (char *)m + kGuard;  // a stack that overflows hits the guard page
    }
  }
  ~Workgroup() {
    for (auto &f : f_) munmap(f.map, kStack + kGuard);
  }
  Workgroup(const Workgroup &) = delete;
  Workgroup &operator=(const Workgroup &) = delete;

  // f(tid, sync) for tid = 0 .. threads - 1 as one workgroup
  template <class F>
  Stats run(Schedule &schedule, long skip, F f) {
    struct Call {
      F *f;
      static void go(void *p, int tid, Sync s) { (*static_cast<Call *>(p)->f)(tid, s); }
    } call{&f};
    call_ = &Call::go, arg_ = &call, skip_ = skip;
    for (int t = 0; t < n_; ++t) {
      Fibre &fb = f_[(size_t)t];
      fb.state = kReady, fb.syncs = 0, fb.fake = nullptr;
      getcontext(&fb.ctx);
      fb.ctx.uc_stack.ss_sp = fb.stack, fb.ctx.uc_stack.ss_size = kStack, fb.ctx.uc_link = nullptr;
      makecontext(&fb.ctx, (void (*)())entry, 0);
    }
    Stats st;
    std::vector<int> order;
    for (int alive = n_; alive;) {
      schedule.order(n_, (uint64_t)st.intervals++, order);
      for (int t : order) {
        if (f_[(size_t)t].state == kDone) continue;
        resume(t);
        if (f_[(size_t)t].state == kDone) --alive;
      }
      if (alive && alive != n_) {
        int d = 0, w = 0;
        while (f_[(size_t)d].state != kDone) ++d;
        while (f_[(size_t)w].state == kDone) ++w;
        diverged(d, f_[(size_t)d].syncs, w, f_[(size_t)w].syncs);
      }
    }
    st.syncs = f_[0].syncs;
    for (int t = 1; t < n_; ++t)
      if (f_[(size_t)t].syncs != st.syncs) diverged(t, f_[(size_t)t].syncs, 0, st.syncs);
    return st;
  }

 private:
  friend struct Sync;
  enum State { kReady, kWaiting, kDone };
  struct Fibre {
    ucontext_t ctx;
    void *map, *stack, *fake;
    State state;
    long syncs;
  };

  static Workgroup *&current() {
    static Workgroup *w = nullptr;
    return w;
  }

  void resume(int t) {
    current() = this, running_ = t;
#if defined(WG_ASAN)
    void *fake = nullptr;
    __sanitizer_start_switch_fiber(&fake, f_[(size_t)t].stack, kStack);
#endif
    swapcontext(&main_, &f_[(size_t)t].ctx);
#if defined(WG_ASAN)
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
  }

  // from the running fibre back to run(); `last`: the fibre has returned and its stack is not used again
  void yield(bool last) {
    Fibre &fb = f_[(size_t)running_];
#if defined(WG_ASAN)
    __sanitizer_start_switch_fiber(last ? nullptr : &fb.fake, main_bottom_, main_size_);
#endif
    swapcontext(&fb.ctx, &main_);
#if defined(WG_ASAN)
    __sanitizer_finish_switch_fiber(fb.fake, &main_bottom_, &main_size_);
#endif
    (void)last;
  }

  static void entry() {
    Workgroup *w = current();
#if defined(WG_ASAN)
    __sanitizer_finish_switch_fiber(nullptr, &w->main_bottom_, &w->main_size_);
#endif
    const int t = w->running_;
    w->call_(w->arg_, t, Sync{w, t});
    w->f_[(size_t)t].state = kDone;
    w->yield(true);
    std::abort();  // a fibre that has returned is not resumed
  }

  void sync(int t) {
    Fibre &fb = f_[(size_t)t];
    if (fb.syncs++ == skip_) return;
    fb.state = kWaiting;
    yield(false);
    fb.state = kReady;
  }

  int n_;
  std::vector<Fibre> f_;
  ucontext_t main_;
  const void *main_bottom_ = nullptr;
  size_t main_size_ = 0;
  int running_ = 0;
  long skip_ = -1;
  void (*call_)(void *, int, Sync) = nullptr;
  void *arg_ = nullptr;
};

inline void Sync::operator()() const { wg->sync(tid); }

#else  // WG_FREE_RUNNING

class Workgroup;
struct Sync {
  Workgroup *wg;
  int tid;
  void operator()() const;
};

class Workgroup {
 public:
  explicit Workgroup(int threads) : n_(threads), syncs_((size_t)threads) {}

  template <class F>
  Stats run(Schedule &, long skip, F f) {
    skip_ = skip, waiting_ = 0, done_ = 0, generation_ = 0;
    std::vector<std::thread> th;
    th.reserve((size_t)n_);
    for (int t = 0; t < n_; ++t) {
      syncs_[(size_t)t] = 0;
      th.emplace_back([this, t, &f] {
        f(t, Sync{this, t});
        std::lock_guard<std::mutex> l(m_);
        ++done_, last_done_ = t;
        if (waiting_) diverged(t, syncs_[(size_t)t], waiter_, syncs_[(size_t)waiter_] - 1);
      });
    }
    for (auto &t : th) t.join();
    Stats st;
    st.syncs = syncs_[0];
    for (int t = 1; t < n_; ++t)
      if (syncs_[(size_t)t] != st.syncs) diverged(t, syncs_[(size_t)t], 0, st.syncs);
    return st;
  }

 private:
  friend struct Sync;
  void sync(int t) {
    if (syncs_[(size_t)t]++ == skip_) return;
    std::unique_lock<std::mutex> l(m_);
    if (done_) diverged(last_done_, syncs_[(size_t)last_done_], t, syncs_[(size_t)t] - 1);
    waiter_ = t;
    if (++waiting_ == n_) {
      waiting_ = 0, ++generation_;
      cv_.notify_all();
      return;
    }
    const uint64_t g = generation_;
    cv_.wait(l, [&] { return generation_ != g; });
  }

  int n_;
  std::vector<long> syncs_;  // each entry written by its own thread; read by others under m_ or after join
  std::mutex m_;
  std::condition_variable cv_;
  int waiting_ = 0, done_ = 0, waiter_ = 0, last_done_ = 0;
  uint64_t generation_ = 0;
  long skip_ = -1;
};

inline void Sync::operator()() const { wg->sync(tid); }

#endif

// device LDS is not initialised: what a tile finds in its buffer
struct Fill {
  enum Kind { kZero, kOnes, kRandom } kind;
  Rng rng;
  Fill() : kind(kZero), rng(0) {}
  static bool parse(const char *name, uint64_t seed, Fill &f) {
    static const char *const n[] = {"zero", "ones", "random"};
    for (int k = 0; k < 3; ++k)
      if (!std::strcmp(name, n[k])) return f.kind = (Kind)k, f.rng = Rng(seed ^ 0x4C4453u), true;
    return false;
  }
  // (random: the stream goes on from tile to tile)
  void apply(uint8_t *p, size_t n) {
    if (kind != kRandom) {
      std::memset(p, kind == kOnes ? 0xFF : 0, n);
      return;
    }
    for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)(rng.next() >> 56);
  }
};

}  // namespace wg
