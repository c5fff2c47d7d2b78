// Deferred weight-gradient work (see wgrad_reduce.h): parked eight-wave launches and the batched reduction of the partial sums.
#include "wgrad_reduce.h"
#include "../core/switches.h"
#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>

namespace lamp {

constexpr int WR_MAX = 16;
struct WgradReduceMany { WgradReduceArgs e[WR_MAX]; };

__global__ __launch_bounds__(256) void wgrad_reduce_many_kernel(WgradReduceMany m) {
  __shared__ float4 red[8][32];
  const WgradReduceArgs& a = m.e[blockIdx.y];
  if ((int)blockIdx.x >= a.blocks) return;          // uniform per workgroup
  if (a.kind == 0) wgrad_reduce_igemm(a, blockIdx.x, red);
  else wgrad_reduce_narrow(a, blockIdx.x);
}

namespace {
// One registry, one mutex.  An entry is a parked eight-wave launch (p.dy set: wgrad_park - its tensors retained, dy / x / affine counted in
// their storages' `deferred_reads`) or a pending reduction (partial set); either way it is counted in dw's storage's `pending`.
// Ownership: an entry belongs to the host thread that registered it.  flush_deferred() - the natural batching point - only
// takes the CALLING thread's entries, so the replica threads of the single-process data-parallel step never flush each other's work;
// resolve_deferred(storage), reached from raw() / data() of any thread, takes the entries of the thread that owns an entry naming that
// storage, and of that thread only.  A flush does all of its work with g_mu held: the entries leave the list, the parked layers are
// launched in the order they were parked, the reductions they leave join the batch, the batch is launched, and only then are the counts
// dropped - a concurrent accessor blocks on the mutex and returns with the work queued in front of whatever it launches next.
struct Entry { Wg8hProblem p; WgradReduceArgs a; Tensor* partial; hipStream_t st; int device; std::thread::id owner; };
std::mutex g_mu;
std::vector<Entry> g_list;

void count_reads(const Wg8hProblem& p, uint32_t d) {
  for (const Tensor* t : {p.dy, p.x, p.affine}) if (t) t->st->deferred_reads.fetch_add(d, std::memory_order_acq_rel);
}
bool names(const Entry& e, const Storage* st) {
  return e.p.dw->st == st || (e.p.dy && (e.p.dy->st == st || e.p.x->st == st || (e.p.affine && e.p.affine->st == st)));
}
// Entries out of the list: when this goes out of scope - launched, or skipped by an exception - their counts are dropped (after the launches
// are queued) and their handles released.  Nothing leaves the list except into one of these.
struct Taken {
  std::vector<Entry> v;
  ~Taken() {
    for (auto& e : v) { e.p.dw->st->pending.fetch_sub(1, std::memory_order_release); if (e.p.dy) count_reads(e.p, (uint32_t)-1); }
    for (auto& e : v) for (const Tensor* t : {e.p.dy, e.p.x, e.p.affine, (const Tensor*)e.p.dw, (const Tensor*)e.partial}) release(const_cast<Tensor*>(t));
  }
};
// called with g_mu held: launches parked layer e (with b) on its stream; the reductions it leaves are appended to `into` as pending entries of e's owner
void wg8h_launch_locked(const Entry e, const Wg8hProblem* b, std::vector<Entry>& into) {
  const int prev = current_device();
  if (prev != e.device) set_device(e.device);
  struct Back { int prev, dev; ~Back() { if (prev != dev) set_device(prev); } } back{prev, e.device};
  std::vector<WgradReduction> out;
  wg8h_launch(e.p, b, e.st, nullptr, &out);
  for (auto& r : out) {
    // another thread's layer: its partial sums come from this thread's stream pool and are used on the owner's stream
    if (e.st != current_stream(e.device)) record_stream(r.partial.get(), e.device, e.st);
    into.push_back(Entry{Wg8hProblem{nullptr, nullptr, r.dw.get(), {}, nullptr}, r.a, r.partial.get(), e.st, e.device, e.owner});
    r.dw->st->pending.fetch_add(1, std::memory_order_release);
    r.dw.take(); r.partial.take();
  }
}

// called with g_mu held: one launch per (device, stream) group of at most WR_MAX pending reductions; order of registration kept.
// Pointers are taken from the storages directly (raw() would recurse into resolve_deferred).
void launch_batch(const std::vector<Entry>& v) {
  std::vector<bool> done(v.size(), false);
  for (size_t i = 0; i < v.size(); i++) {
    if (done[i] || !v[i].partial) continue;
    WgradReduceMany m;
    int cnt = 0, maxb = 0;
    for (size_t j = i; j < v.size() && cnt < WR_MAX; j++) {
      if (done[j] || !v[j].partial || v[j].st != v[i].st || v[j].device != v[i].device) continue;
      m.e[cnt] = v[j].a;
      m.e[cnt].partial = reinterpret_cast<const float*>(static_cast<const char*>(v[j].partial->st->ptr)) + v[j].partial->offset;
      m.e[cnt].dw = static_cast<char*>(v[j].p.dw->st->ptr) + v[j].p.dw->offset * (v[j].a.dw_f32 ? 4 : 2);
      v[j].p.dw->st->version.fetch_add(1, std::memory_order_relaxed);   // a writer like any other: bumps dw's version
      maxb = std::max(maxb, v[j].a.blocks);
      done[j] = true;
      cnt++;
    }
    const int prev = current_device();
    if (prev != v[i].device) set_device(v[i].device);
    hipLaunchKernelGGL(wgrad_reduce_many_kernel, dim3((unsigned)maxb, (unsigned)cnt), dim3(256), 0, v[i].st, m);
    hipError_t e = hipGetLastError();
    if (prev != v[i].device) set_device(prev);
    if (e != hipSuccess) throw Error(std::string("wgrad reduce launch failed: ") + hipGetErrorString(e));
    // a reader on another stream of that device must see the result: order it behind the reduction (and the parked launch in front of it)
    hipStream_t cur = current_stream(v[i].device);
    if (cur != v[i].st) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (allocator_capturing()) HIP_CHECK(hipStreamIsCapturing(v[i].st, &cs));
      if (allocator_capturing() && cs != hipStreamCaptureStatusActive) {
        // the caller is recording a graph on `cur` and the reduction's stream is outside that capture: an event from outside the capture
        // cannot be waited for inside it - wait on the host.  (A stream forked INTO the capture - the weight gradients' second stream,
        // host/ops.cpp - is joined with an event like any other: both ends are nodes of the same graph.)
        HIP_CHECK(hipStreamSynchronize(v[i].st));
      } else {
        hipEvent_t ev;
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(ev, v[i].st));
        HIP_CHECK(hipStreamWaitEvent(cur, ev, 0));
        HIP_CHECK(hipEventDestroy(ev));
      }
    }
  }
}

// takes the entries of `owner` out of the list, launches its parked layers and then the batch, drops the counts - all under g_mu
void flush_owner_locked(std::thread::id owner) {
  Taken t;
  size_t keep = 0;
  for (size_t i = 0; i < g_list.size(); i++) {
    if (g_list[i].owner == owner) t.v.push_back(g_list[i]);
    else g_list[keep++] = g_list[i];
  }
  g_list.resize(keep);
  const size_t n = t.v.size();
  for (size_t i = 0; i < n; i++)
    if (t.v[i].p.dy) wg8h_launch_locked(t.v[i], nullptr, t.v);
  launch_batch(t.v);
}
}  // namespace

void flush_deferred() {
  std::lock_guard<std::mutex> lk(g_mu);
  flush_owner_locked(std::this_thread::get_id());
}

void resolve_deferred(Storage* st) {
  std::lock_guard<std::mutex> lk(g_mu);
  // every owner of an entry naming st (one input may be read by several threads' parked layers); none: already queued by another thread
  auto hit = [&] { return std::find_if(g_list.begin(), g_list.end(), [&](const Entry& e) { return names(e, st); }); };
  for (auto it = hit(); it != g_list.end(); it = hit()) flush_owner_locked(it->owner);
}

void wgrad_park(const Wg8hProblem& p, hipStream_t st) {
  (void)p.dy->raw(); (void)p.x->raw();          // (their own deferred work, if any, first: a launch under g_mu must not resolve anything)
  const int dev = p.dw->device();
  const std::thread::id me = std::this_thread::get_id();
  std::lock_guard<std::mutex> lk(g_mu);
  auto m = std::find_if(g_list.begin(), g_list.end(), [&](const Entry& e) {
    return e.p.dy && e.owner == me && e.st == st && e.device == dev && e.p.g.N == p.g.N && e.p.dw->st != p.dw->st;
  });
  if (m != g_list.end()) {                      // the mate: both layers in one launch
    Taken t{{*m}};
    g_list.erase(m);
    wg8h_launch_locked(t.v[0], &p, g_list);
    return;
  }
  Entry e{Wg8hProblem{retain(p.dy), retain(p.x), retain(p.dw), p.g, p.affine ? retain(p.affine) : nullptr}, {}, nullptr, st, dev, me};
  g_list.push_back(e);
  count_reads(e.p, 1);
  p.dw->st->version.fetch_add(1, std::memory_order_relaxed);  // a writer like any other
  p.dw->st->pending.fetch_add(1, std::memory_order_release);
}

bool wgrad_reduce_deferred() {
  const bool defer = sw().defer_wgrad_reduce;
  return defer;
}
void wgrad_reduce_enqueue(const WgradReduceArgs& a, lamp_tensor* partial, lamp_tensor* dw, hipStream_t st) {
  const bool defer = wgrad_reduce_deferred();
  if (!defer || !dw->st->owned) {
    WgradReduceMany m;
    m.e[0] = a;
    m.e[0].cached = defer ? 0 : 1;
    m.e[0].partial = partial->ptr<float>();
    m.e[0].dw = dw->data();
    hipLaunchKernelGGL(wgrad_reduce_many_kernel, dim3((unsigned)a.blocks, 1), dim3(256), 0, st, m);
    LAMP_LAUNCH_CHECK();
    return;
  }
  Entry e{Wg8hProblem{nullptr, nullptr, retain(dw), {}, nullptr}, a, retain(partial), st, dw->device(), std::this_thread::get_id()};
  std::lock_guard<std::mutex> lk(g_mu);
  g_list.push_back(e);
  dw->st->pending.fetch_add(1, std::memory_order_release);
}
void wgrad_reduce_flat(int O, int nsplit, lamp_tensor* partial, lamp_tensor* dw, hipStream_t st, bool dw_f32) {
  WgradReduceArgs ra{};
  ra.kind = 1; ra.O = O; ra.nsplit = nsplit; ra.dw_f32 = dw_f32 ? 1 : 0;
  ra.blocks = (int)(((int64_t)O * 64 + 255) / 256);          // a wave per output
  wgrad_reduce_enqueue(ra, partial, dw, st);
}

}  // namespace lamp
