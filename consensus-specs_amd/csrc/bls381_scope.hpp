// Scope-bound stream forks and held host data of the C-ABI host layer (bls381_capi.hip): every
// way out of a scope -- the last line, an error return, an exception -- does what the success
// path does.
//
// Host only and without a HIP include: written against hipStream_t, hipEvent_t, hipError_t and the
// runtime calls named below, which the including file declares first -- bls381_capi.hip with
// <hip/hip_runtime.h>, host_check.cpp with stand-ins that append to a call log.  Everything here
// has internal linkage, so the two libraries, loaded into one process, never share a definition
// that is bound to the other's calls.
//
//   hipStreamCreateWithFlags  hipStreamCreateWithPriority  hipDeviceGetStreamPriorityRange
//   hipStreamSynchronize  hipStreamWaitEvent  hipStreamDestroy
//   hipEventCreateWithFlags  hipEventRecord  hipEventQuery  hipEventDestroy
#pragma once
#include <deque>
#include <memory>
#include <mutex>
#include <utility>

namespace bls381 {
namespace {

// A side stream owns the event that marks its branch of a fork complete.
struct Side {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
};

// A context's streams: the context stream of the host-pointer entry points, and the side streams
// on which independent stages of one batch run beside the caller's stream (a Fork, below).
struct Streams {
  hipStream_t main = nullptr;
  Side side, side2;
  // high priority: small latency-bound launches whose waves should be dispatched ahead of a
  // large launch queued at the same time on another stream
  Side prio;
  hipEvent_t fork = nullptr;
  std::mutex fork_mu;   // one fork at a time uses the side streams and their events
};

// Destroys whatever of `q` exists (after a failed streams_create: what was made before the failure).
inline void streams_destroy(Streams& q) {
  for (Side* sd : {&q.side, &q.side2, &q.prio}) {
    if (sd->stream) {
      (void)hipStreamSynchronize(sd->stream);
      (void)hipStreamDestroy(sd->stream);
    }
    if (sd->done) (void)hipEventDestroy(sd->done);
    *sd = Side();
  }
  if (q.fork) (void)hipEventDestroy(q.fork);
  if (q.main) (void)hipStreamDestroy(q.main);
  q.fork = nullptr;
  q.main = nullptr;
}

inline hipError_t streams_create(Streams& q) {
  int prio_lo = 0, prio_hi = 0;
  hipError_t e = hipStreamCreateWithFlags(&q.main, hipStreamNonBlocking);
  for (Side* sd : {&q.side, &q.side2}) {
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&sd->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sd->done, hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&q.prio.stream, hipStreamNonBlocking, prio_hi);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&q.prio.done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&q.fork, hipEventDisableTiming);
  if (e != hipSuccess) streams_destroy(q);
  return e;
}

// A fork of `main` onto side streams, with fork_mu held for its lifetime.  branch(side) makes the
// side stream wait for everything queued on `main` at the fork point (the first branch); join()
// makes `main` wait for everything queued on the branched streams since.  The destructor joins what
// is still open, so no exit leaves side-stream work on the caller's workspace that the caller's
// stream does not wait for.
class Fork {
 public:
  Fork(Streams& q, hipStream_t main) : q_(q), main_(main), lk_(q.fork_mu) {}
  Fork(const Fork&) = delete;
  Fork& operator=(const Fork&) = delete;
  ~Fork() { (void)join(); }

  hipError_t branch(Side& sd) {
    if (!forked_) {
      const hipError_t e = hipEventRecord(q_.fork, main_);
      if (e != hipSuccess) return e;
      forked_ = true;
    }
    const hipError_t e = hipStreamWaitEvent(sd.stream, q_.fork, 0);
    if (e == hipSuccess) open_[n_open_++] = &sd;
    return e;
  }

  // Every open branch is joined whatever happens to the others; the first error is returned (by
  // every later join() too).  A branch that cannot be joined in stream order is waited for here.
  hipError_t join() {
    for (int i = 0; i < n_open_; ++i) {
      hipError_t e = hipEventRecord(open_[i]->done, open_[i]->stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(main_, open_[i]->done, 0);
      if (e != hipSuccess) {
        (void)hipStreamSynchronize(open_[i]->stream);
        if (err_ == hipSuccess) err_ = e;
      }
    }
    n_open_ = 0;
    return err_;
  }

 private:
  Streams& q_;
  hipStream_t main_;
  std::lock_guard<std::mutex> lk_;
  Side* open_[3] = {nullptr, nullptr, nullptr};   // each side stream branches at most once
  int n_open_ = 0;
  bool forked_ = false;
  hipError_t err_ = hipSuccess;
};

// Host memory that an async copy still reads: released once an event recorded after the copy has
// completed (device-pointer entry points return without synchronising, so a plan on the C++ stack
// would die too early).
struct Keep {
  hipEvent_t ev = nullptr;
  std::shared_ptr<void> data;
};
struct KeepList {
  std::mutex mu;
  std::deque<Keep> items;
};

// Keeps `data` alive until the work queued on `s` so far has completed: parked behind an event, or,
// when no event can be had, by waiting for the stream here.
inline void keep_until_done(KeepList& k, hipStream_t s, std::shared_ptr<void> data) noexcept {
  try {
    std::lock_guard<std::mutex> lk(k.mu);
    while (!k.items.empty() && hipEventQuery(k.items.front().ev) == hipSuccess) {
      (void)hipEventDestroy(k.items.front().ev);
      k.items.pop_front();
    }
    k.items.emplace_back();   // the one step that can throw, before there is an event to lose
    Keep& slot = k.items.back();
    if (hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming) == hipSuccess) {
      if (hipEventRecord(slot.ev, s) == hipSuccess) {
        slot.data = std::move(data);
        return;
      }
      (void)hipEventDestroy(slot.ev);
    }
    k.items.pop_back();
  } catch (...) {
  }
  (void)hipStreamSynchronize(s);
}

// Releases everything (the caller has synchronised the device).
inline void keep_clear(KeepList& k) {
  std::lock_guard<std::mutex> lk(k.mu);
  for (Keep& e : k.items) (void)hipEventDestroy(e.ev);
  k.items.clear();
}

// A value that copies queued on `s` during this scope read: declared where the value is made, and
// handed to keep_until_done however the scope is left.
template <class T>
class Held {
 public:
  Held(KeepList& k, hipStream_t s, T&& v) : k_(k), s_(s), p_(std::make_shared<T>(std::move(v))) {}
  Held(const Held&) = delete;
  Held& operator=(const Held&) = delete;
  ~Held() { keep_until_done(k_, s_, std::move(p_)); }
  T& operator*() const { return *p_; }
  T* operator->() const { return p_.get(); }

 private:
  KeepList& k_;
  hipStream_t s_;
  std::shared_ptr<T> p_;
};

}  // namespace
}  // namespace bls381
