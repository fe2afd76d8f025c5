// Python bindings for the rdp HIP kernels (built in-tree as robotic_discovery_platform_amd/_C.so).
//
// Activations are NHWC bf16 torch tensors ([N,H,W,C], channel stride 1, possibly a channel slice
// of a wider tensor: pixel pitch = stride(2)). Every launcher validates shapes/strides here so a
// kernel never sees an inconsistent view; the kernels themselves use buffer descriptors sized from
// these views (out-of-range = zero / dropped, never a fault).
//
// The launchers (rdp_*) are declared once, with named parameters and their contracts, in csrc/rdp_api.h (GPU)
// and csrc/rdp_host_api.h (host codecs / spline): no prototype is written here.
#include <torch/extension.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <link.h>
#include <chrono>
#include <cmath>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>
#include <array>

#include "bn_dev.h"
#include "rdp_api.h"

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// ---- device placement: every binding runs on the GPU that holds its tensors -------------------------
// `on_device(fn)` wraps a binding: it checks that every GPU tensor argument (plain or optional) lives
// on ONE device and makes that device current for the call (HIPGuard), so the launches below go to
// that device's current stream -- a per-GPU serving replica (serve/engine.py EnginePool) launches on
// its own GPU whatever device the calling thread had current. Mixed devices raise.
void note_device(int& dev, const torch::Tensor& t) {
  if (!t.defined() || !t.is_cuda()) return;
  const int d = t.get_device();
  TORCH_CHECK(dev < 0 || d == dev, "tensor arguments on different GPUs (cuda:", dev, " and cuda:", d, ")");
  dev = d;
}
void note_device(int& dev, const c10::optional<torch::Tensor>& t) {
  if (t) note_device(dev, *t);
}
void note_device(int& dev, const std::vector<torch::Tensor>& ts) {
  for (const auto& t : ts) note_device(dev, t);
}
template <class T>
void note_device(int&, const T&) {}

template <class R, class... A>
auto on_device(R (*fn)(A...)) {
  return [fn](A... args) -> R {
    int dev = -1;
    (note_device(dev, args), ...);
    c10::hip::OptionalHIPGuard guard;
    if (dev >= 0) guard.set_index((c10::DeviceIndex)dev);
    return fn(std::move(args)...);
  };
}

// ---- launch plans: the training step recorded once and replayed from C++ --------------------------
// A plan is the step's launch sequence: every kernel launch of the bindings below (RDP_PLAN) and every
// cross-stream dependency (stream_wait), in issue order, each with the HIP stream it was issued on.
// Recording runs the step normally and keeps, per launch, a closure over the already-validated raw
// arguments (pointers into the executor's static buffers, ints); replay re-issues the closures on
// the recorded streams -- about 1-2 us of host time per launch instead of the Python executor's
// ~8 us, so at small batch the host stays ahead of the GPU (bs 4: 1.55 ms of host enqueue per 2.5 ms
// step, with idle gaps wherever a run of short kernels outpaced it). Unlike a hipGraph, replay keeps
// the eager launch order on the same two streams / hardware queues (graph replay spread the side
// branch over extra queues and measured slower, train/engine.py).
//
// A plan may also hold host call points (kind 2, ``plan_mark``): work the runtime cannot replay itself
// (the DDP bucket all-reduces, issued through torch.distributed). Recording marks the point, then runs
// that work with recording paused (``plan_pause`` / ``plan_resume``); replay calls back into Python with
// the mark's tag at the same position in the launch sequence, so the collectives keep their place
// between the recorded kernels.
struct PlanOp {
  int kind;        // 0: launch, 1: waiter waits for everything issued so far on waitee, 2: host call,
                   // 3: record a runtime-owned event on s, 4: s waits for that event's last record
  hipStream_t s;   // launch stream / waiter
  hipStream_t s2;  // waitee
  hipEvent_t ev;
  std::function<long(hipStream_t)> fn;
  int tag = -1;    // kind 2: the caller's call-point id
};
struct Plan {
  std::vector<PlanOp> ops;
};
std::vector<std::unique_ptr<Plan>> g_plans;
Plan* g_rec = nullptr;
Plan* g_paused = nullptr;  // the plan being recorded while a host call point runs

template <class F>
long plan_launch(F&& f) {
  const hipStream_t s = cur_stream();
  if (g_rec) g_rec->ops.push_back(PlanOp{0, s, nullptr, nullptr, std::function<long(hipStream_t)>(f)});
  return f(s);
}
#define RDP_PLAN(...) plan_launch([=](hipStream_t st) -> long { return (long)(__VA_ARGS__); })

// launches that a plan cannot hold (serving / geometry bindings): refuse while recording
hipStream_t unplanned_stream() {
  TORCH_CHECK(g_rec == nullptr, "this kernel launch cannot be recorded into a plan");
  return cur_stream();
}

// One reusable timing-free event per device and host thread for the eager path: hipStreamWaitEvent
// captures the event's most recent record at the time of the call, so re-recording it for the next
// wait is safe (no create / destroy per call). A plan being recorded owns one event per wait.
// Cross-stream dependencies on one GPU only order kernels, and every kernel dispatch already carries its
// own acquire / release fences, so the events skip the system-scope fence (L2 writeback for host
// visibility) that a default event record inserts into the waitee's queue: bs 4 step 2.50-2.53 ->
// 2.48 ms (1,584-1,601 -> 1,615 img/s, 2 rounds, same box; a device-scope release instead: no change;
// bs 64 neutral).
static unsigned wait_event_flags() { return hipEventDisableTiming | hipEventDisableSystemFence; }

hipEvent_t wait_event(hipStream_t s) {
  int dev = 0;
  TORCH_CHECK(hipStreamGetDevice(s, &dev) == hipSuccess, "stream_wait: stream device");
  thread_local std::vector<hipEvent_t> evs;
  if ((int)evs.size() <= dev) evs.resize(dev + 1, nullptr);
  if (!evs[dev]) {
    c10::hip::HIPGuard g((c10::DeviceIndex)dev);
    TORCH_CHECK(hipEventCreateWithFlags(&evs[dev], wait_event_flags()) == hipSuccess, "stream_wait: event");
  }
  return evs[dev];
}

void stream_wait(long waiter, long waitee) {
  const hipStream_t w = (hipStream_t)waiter, e = (hipStream_t)waitee;
  hipEvent_t ev;
  if (g_rec) {
    int dev = 0;
    TORCH_CHECK(hipStreamGetDevice(e, &dev) == hipSuccess, "stream_wait: stream device");
    c10::hip::HIPGuard g((c10::DeviceIndex)dev);
    TORCH_CHECK(hipEventCreateWithFlags(&ev, wait_event_flags()) == hipSuccess, "stream_wait: event");
  } else {
    ev = wait_event(e);
  }
  TORCH_CHECK(hipEventRecord(ev, e) == hipSuccess && hipStreamWaitEvent(w, ev, 0) == hipSuccess, "stream_wait");
  if (g_rec) g_rec->ops.push_back(PlanOp{1, w, e, ev, nullptr});
}

// Named cross-stream points (runtime-owned events, recorded into plans): event_record marks "everything
// issued so far on this stream", stream_wait_event makes another stream wait for the LAST such mark --
// a dependency on a point in the middle of a stream's work (NativeAdam's overlapped update: the next
// forward waits for the update, not for the weight re-layouts queued behind it).
std::vector<hipEvent_t> g_events;

int event_create() {
  hipEvent_t e;
  TORCH_CHECK(hipEventCreateWithFlags(&e, wait_event_flags()) == hipSuccess, "event_create");
  g_events.push_back(e);
  return (int)g_events.size() - 1;
}

void event_record(int id, long stream) {
  TORCH_CHECK(id >= 0 && id < (int)g_events.size(), "event_record: bad event id");
  const hipStream_t s = (hipStream_t)stream;
  TORCH_CHECK(hipEventRecord(g_events[id], s) == hipSuccess, "event_record");
  if (g_rec) g_rec->ops.push_back(PlanOp{3, s, nullptr, g_events[id], nullptr});
}

void stream_wait_event(long stream, int id) {
  TORCH_CHECK(id >= 0 && id < (int)g_events.size(), "stream_wait_event: bad event id");
  const hipStream_t s = (hipStream_t)stream;
  TORCH_CHECK(hipStreamWaitEvent(s, g_events[id], 0) == hipSuccess, "stream_wait_event");
  if (g_rec) g_rec->ops.push_back(PlanOp{4, s, nullptr, g_events[id], nullptr});
}

void plan_begin() {
  TORCH_CHECK(g_rec == nullptr && g_paused == nullptr, "plan_begin: already recording");
  g_plans.emplace_back(new Plan());
  g_rec = g_plans.back().get();
}

int plan_end() {
  TORCH_CHECK(g_rec != nullptr, "plan_end: not recording");
  g_rec = nullptr;
  return (int)g_plans.size() - 1;
}

void plan_abort() {
  if (g_paused) {
    g_rec = g_paused;
    g_paused = nullptr;
  }
  if (g_rec) {
    for (auto& op : g_rec->ops) if (op.ev && op.kind == 1) hipEventDestroy(op.ev);
    g_rec->ops.clear();
    g_rec = nullptr;
  }
}

bool plan_recording() { return g_rec != nullptr; }

void plan_mark(int tag) {
  TORCH_CHECK(g_rec != nullptr, "plan_mark: not recording");
  PlanOp op{2, nullptr, nullptr, nullptr, nullptr};
  op.tag = tag;
  g_rec->ops.push_back(std::move(op));
}

void plan_pause() {
  TORCH_CHECK(g_rec != nullptr && g_paused == nullptr, "plan_pause: not recording");
  g_paused = g_rec;
  g_rec = nullptr;
}

void plan_resume() {
  TORCH_CHECK(g_paused != nullptr && g_rec == nullptr, "plan_resume: not paused");
  g_rec = g_paused;
  g_paused = nullptr;
}

void plan_replay(int id, py::object host_call) {
  TORCH_CHECK(id >= 0 && id < (int)g_plans.size() && g_plans[id], "plan_replay: bad plan id");
  TORCH_CHECK(g_rec == nullptr && g_paused == nullptr, "plan_replay while recording");
  for (auto& op : g_plans[id]->ops) {
    if (op.kind == 0) {
      op.fn(op.s);
    } else if (op.kind == 1) {
      hipEventRecord(op.ev, op.s2);
      hipStreamWaitEvent(op.s, op.ev, 0);
    } else if (op.kind == 3) {
      hipEventRecord(op.ev, op.s);
    } else if (op.kind == 4) {
      hipStreamWaitEvent(op.s, op.ev, 0);
    } else {
      TORCH_CHECK(!host_call.is_none(), "plan_replay: the plan has host call points, pass a callback");
      host_call(op.tag);
    }
  }
}

int plan_size(int id) {
  TORCH_CHECK(id >= 0 && id < (int)g_plans.size() && g_plans[id], "plan_size: bad plan id");
  return (int)g_plans[id]->ops.size();
}

// the op kinds of a recorded plan, in order (tests: which cross-stream waits a plan holds)
std::vector<int> plan_kinds(int id) {
  TORCH_CHECK(id >= 0 && id < (int)g_plans.size() && g_plans[id], "plan_kinds: bad plan id");
  std::vector<int> k;
  for (auto& op : g_plans[id]->ops) k.push_back(op.kind);
  return k;
}

void plan_free(int id) {
  if (id < 0 || id >= (int)g_plans.size() || !g_plans[id]) return;
  for (auto& op : g_plans[id]->ops) if (op.ev && op.kind == 1) hipEventDestroy(op.ev);
  g_plans[id].reset();
}

// ---- RCCL collectives enqueued straight onto HIP streams ---------------------------------------------
// The DDP gradient buckets are all-reduced with ncclAllReduce on the communicator of a dedicated
// torch.distributed (nccl = RCCL) process group (ProcessGroupNCCL._comm_ptr), issued on the executor's
// stream in stream order -- no ProcessGroupNCCL work objects, events or host waits per bucket -- and
// recorded into launch plans like a kernel launch, so a DDP step replays from C++ with its collectives
// in place. The entry points are resolved from the librccl instance torch itself loaded (the
// communicator belongs to it), never from another copy of the library.
typedef int (*NcclAllReduceFn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*NcclAsyncErrFn)(void*, int*);
typedef const char* (*NcclErrStrFn)(int);
typedef int (*NcclAbortFn)(void*);
typedef int (*NcclCommIntFn)(const void*, int*);
struct RcclApi {
  NcclAllReduceFn all_reduce = nullptr;
  NcclAsyncErrFn async_err = nullptr;
  NcclErrStrFn err_str = nullptr;
  NcclAbortFn abort = nullptr;
  NcclCommIntFn count = nullptr, user_rank = nullptr, device = nullptr;
  std::string path;
} g_rccl;

int find_loaded_rccl(struct dl_phdr_info* info, size_t, void* out) {
  if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) {
    *(std::string*)out = info->dlpi_name;
    return 1;
  }
  return 0;
}

std::string comm_bind() {
  if (g_rccl.all_reduce) return g_rccl.path;
  std::string path;
  dl_iterate_phdr(find_loaded_rccl, &path);
  TORCH_CHECK(!path.empty(), "comm_bind: RCCL is not loaded in this process (create the nccl process group first)");
  void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_NOLOAD);
  TORCH_CHECK(h != nullptr, "comm_bind: dlopen ", path);
  g_rccl.all_reduce = (NcclAllReduceFn)dlsym(h, "ncclAllReduce");
  g_rccl.async_err = (NcclAsyncErrFn)dlsym(h, "ncclCommGetAsyncError");
  g_rccl.err_str = (NcclErrStrFn)dlsym(h, "ncclGetErrorString");
  g_rccl.abort = (NcclAbortFn)dlsym(h, "ncclCommAbort");
  g_rccl.count = (NcclCommIntFn)dlsym(h, "ncclCommCount");
  g_rccl.user_rank = (NcclCommIntFn)dlsym(h, "ncclCommUserRank");
  g_rccl.device = (NcclCommIntFn)dlsym(h, "ncclCommCuDevice");
  TORCH_CHECK(g_rccl.count && g_rccl.user_rank && g_rccl.device &&
              g_rccl.all_reduce && g_rccl.async_err && g_rccl.err_str && g_rccl.abort, "comm_bind: RCCL symbols in ",
              path);
  g_rccl.path = path;
  return path;
}

long rccl_check(int r, void* comm) {
  constexpr int kInProgress = 7;  // ncclInProgress: a non-blocking communicator is still enqueuing
  // bounded: the communicators are created blocking (parallel/ddp.py), so this loop should never
  // spin; if one does, fail after RDP_DIST_TIMEOUT_S instead of hanging the issuing thread
  static const double limit_s = [] {
    const char* v = std::getenv("RDP_DIST_TIMEOUT_S");
    return v ? std::atof(v) : 600.0;
  }();
  const auto t0 = std::chrono::steady_clock::now();
  while (r == kInProgress) {
    int e = 0;
    g_rccl.async_err(comm, &e);
    r = e;
    if (r == kInProgress &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) {
      g_rccl.abort(comm);
      TORCH_CHECK(false, "ncclAllReduce: still in progress after ", limit_s, " s; communicator aborted");
    }
  }
  TORCH_CHECK(r == 0, "ncclAllReduce: ", g_rccl.err_str(r));
  return 0;
}

// in-place SUM all-reduce of `buf` (fp32 or bf16) over `comm`, on the current stream
void comm_all_reduce(torch::Tensor buf, long comm) {
  TORCH_CHECK(g_rccl.all_reduce != nullptr, "comm_all_reduce: call comm_bind() first");
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous(), "comm_all_reduce: contiguous device tensor");
  const int dt = buf.scalar_type() == torch::kFloat      ? 7
                 : buf.scalar_type() == torch::kBFloat16 ? 9
                 : buf.scalar_type() == torch::kDouble   ? 8
                                                         : -1;
  TORCH_CHECK(dt >= 0 && comm != 0, "comm_all_reduce: fp32 / bf16 / fp64 buffer and a communicator");
  void* const p = buf.data_ptr();
  const size_t n = (size_t)buf.numel();
  void* const c = (void*)comm;
  const NcclAllReduceFn fn = g_rccl.all_reduce;
  RDP_PLAN(rccl_check(fn(p, p, n, dt, /*ncclSum*/ 0, c, st), c));
}

// SyncBN: fold buf's [rows][width] fp32 partial rows into `out` (width fp64 sums) / write fp64 sums back as
// hi + lo fp32 rows; both recorded in plans
void rows_fold(torch::Tensor buf, int rows, int width, torch::Tensor out) {
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == torch::kFloat && buf.is_contiguous() &&
              (long)rows * width <= buf.numel() && rows >= 1 && width >= 1, "rows_fold: fp32 buffer of rows x width");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kDouble && out.is_contiguous() && out.numel() >= width,
              "rows_fold: fp64 out");
  const float* p = buf.data_ptr<float>();
  double* o = out.data_ptr<double>();
  RDP_PLAN(rdp_rows_fold(p, rows, width, o, st));
}

void rows_hilo(torch::Tensor in, torch::Tensor buf, int width) {
  TORCH_CHECK(in.is_cuda() && in.scalar_type() == torch::kDouble && in.is_contiguous() && in.numel() >= width,
              "rows_hilo: fp64 sums");
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == torch::kFloat && buf.is_contiguous() && buf.numel() >= 2l * width,
              "rows_hilo: fp32 buffer of 2 rows");
  const double* i = in.data_ptr<double>();
  float* b = buf.data_ptr<float>();
  RDP_PLAN(rdp_rows_hilo(i, b, width, st));
}

// ncclCommGetAsyncError of `comm` (0 = healthy) and its message: polled by the host watchdog
// (parallel/watchdog.py) while natively issued collectives are outstanding -- they have no
// ProcessGroupNCCL work objects, so c10d's own watchdog never sees them.
py::tuple comm_async_error(long comm) {
  TORCH_CHECK(g_rccl.async_err != nullptr && comm != 0, "comm_async_error: call comm_bind() first");
  int e = 0;
  const int r = g_rccl.async_err((void*)comm, &e);
  const int code = r != 0 ? r : e;
  return py::make_tuple(code, std::string(code ? g_rccl.err_str(code) : ""));
}

// (ranks, this rank, device) of `comm` as RCCL itself sees them (ncclCommCount / ncclCommUserRank /
// ncclCommCuDevice): bench.py's self-check that the gradient communicator spans WORLD_SIZE ranks
py::tuple comm_info(long comm) {
  TORCH_CHECK(g_rccl.count != nullptr && comm != 0, "comm_info: call comm_bind() first");
  int n = -1, r = -1, d = -1;
  TORCH_CHECK(g_rccl.count((void*)comm, &n) == 0, "ncclCommCount failed");
  TORCH_CHECK(g_rccl.user_rank((void*)comm, &r) == 0, "ncclCommUserRank failed");
  TORCH_CHECK(g_rccl.device((void*)comm, &d) == 0, "ncclCommCuDevice failed");
  return py::make_tuple(n, r, d);
}

// ncclCommAbort: unblocks every kernel of the communicator still waiting on a dead peer (the watchdog's
// last step before it exits the process)
int comm_abort(long comm) {
  TORCH_CHECK(g_rccl.abort != nullptr && comm != 0, "comm_abort: call comm_bind() first");
  py::gil_scoped_release nogil;
  return g_rccl.abort((void*)comm);
}

// RDP_DDP_EMULATE: the modelled all-reduce (`us` microseconds, `blocks` resident workgroups) on the current
// stream in place of ncclAllReduce (csrc/comm.hip), recorded into plans like the real call
// with `scratch` and traffic_bytes > 0: the modelled collective's HBM traffic too (traffic_bytes read from
// the scratch's first half and written to its second, paced over the duration)
void comm_emulate(double us, int blocks, c10::optional<torch::Tensor> scratch, long traffic_bytes) {
  TORCH_CHECK(us >= 0 && blocks >= 1 && blocks <= 4096, "comm_emulate: bad duration / block count");
  if (scratch && traffic_bytes > 0) {
    TORCH_CHECK(scratch->is_cuda() && scratch->is_contiguous() &&
                    scratch->numel() * scratch->element_size() >= 2 * traffic_bytes,
                "comm_emulate: scratch must hold 2 x traffic_bytes");
    void* const p = scratch->data_ptr();
    const long nb = scratch->numel() * scratch->element_size();
    TORCH_CHECK(RDP_PLAN(rdp_comm_emulate_traffic(us, blocks, p, nb, traffic_bytes, st)) == 0, "comm_emulate_traffic");
    return;
  }
  RDP_PLAN(rdp_comm_emulate(us, blocks, st));
}

struct Act {
  void* ptr = nullptr;
  int N = 0, H = 0, W = 0, C = 0, pitch = 0;
  long bytes = 0;
  long image_bytes() const { return (long)H * W * pitch * 2; }            // from one image to the next
  void* image(int n) const { return (char*)ptr + n * image_bytes(); }     // image n
  long span_bytes(int n) const { return ((long)n * H * W - 1) * pitch * 2 + (long)C * 2; }  // extent of n images
};

Act act(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, ": must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, ": must be bf16");
  TORCH_CHECK(t.dim() == 4, name, ": must be NHWC 4-D");
  Act a;
  a.N = t.size(0); a.H = t.size(1); a.W = t.size(2); a.C = t.size(3);
  TORCH_CHECK(t.stride(3) == 1, name, ": channel stride must be 1");
  a.pitch = t.stride(2);
  TORCH_CHECK(a.pitch >= a.C, name, ": pixel pitch < C");
  TORCH_CHECK(t.stride(1) == (long)a.W * a.pitch && t.stride(0) == (long)a.H * a.W * a.pitch, name,
              ": pixels must be densely packed (only channel slicing allowed)");
  TORCH_CHECK(a.pitch % 8 == 0 && ((uintptr_t)t.data_ptr() % 16) == 0, name, ": pitch/base must be 16-B aligned");
  a.ptr = t.data_ptr();
  a.bytes = a.span_bytes(a.N);
  return a;
}

// Images per launch so that every tensor of the launch stays below 2 GiB (the conv kernels' 32-bit
// buffer offsets). RDP_CONV_CHUNK_BYTES (tests) lowers the bound to exercise the chunked path.
int chunk_images(long bytes_per_image, int N) {
  static const long lim = [] {
    const char* e = getenv("RDP_CONV_CHUNK_BYTES");
    const long v = e ? atol(e) : 0L;
    return v > 0 ? v : (1L << 31) - 1;
  }();
  if (bytes_per_image <= 0 || bytes_per_image * N <= lim) return N > 0 ? N : 1;
  return (int)std::max(1L, lim / bytes_per_image);
}

// Images per launch so that each of `ts` stays below 2 GiB (an undefined optional Act counts as empty)
int chunk_images(std::initializer_list<Act> ts, int N) {
  long per_img = 0;
  for (const Act& t : ts) per_img = std::max(per_img, t.image_bytes());
  return chunk_images(per_img, N);
}

// One source or destination of a conv operand block = images [n0, n0 + nn) of t; x1 also sets the block's
// N / H / W, y1 the channel split. An undefined optional Act leaves its slot empty.
enum ConvSlot { kX1, kX2, kY1, kY2 };
void conv_bind(RdpConv& c, ConvSlot slot, const Act& t, int n0, int nn) {
  if (!t.ptr) return;
  void* const p = t.image(n0);
  const long b = t.span_bytes(nn);
  switch (slot) {
    case kX1: c.x1 = p; c.xbytes1 = b; c.C1 = t.C; c.pitch1 = t.pitch; c.N = nn; c.H = t.H; c.W = t.W; break;
    case kX2: c.x2 = p; c.xbytes2 = b; c.C2 = t.C; c.pitch2 = t.pitch; break;
    case kY1: c.y1 = p; c.ybytes1 = b; c.Cy1 = t.C; c.ypitch1 = t.pitch; break;
    case kY2: c.y2 = p; c.ybytes2 = b; c.ypitch2 = t.pitch; break;
  }
}

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous(), name,
              ": must be a contiguous fp32 GPU tensor");
}

void check_w(const torch::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 && w.is_contiguous() && w.dim() == 2,
              "w: bf16 [Cout][K]");
}

// the OHWI weights of a conv operand block
void conv_weights(RdpConv& c, const torch::Tensor& w) {
  check_w(w);
  c.w = w.data_ptr();
  c.wbytes = w.numel() * 2;
  c.ldw = (int)w.size(1);
}

// reduction workspace for the two-stage BN finalize (>= 64 rows x K floats), or nullptr
float* ws_ptr(const c10::optional<torch::Tensor>& ws, int K) {
  if (!ws) return nullptr;
  check_f32(*ws, "ws");
  TORCH_CHECK(ws->numel() >= 64l * K, "workspace too small");
  return ws->data_ptr<float>();
}

// The plan of a dense conv of this shape, as a dict (kernel: the RdpConvKernel value, -1 = unsupported). chunks: the
// image slices conv_fwd / conv_dgrad run a batch past the 2 GiB reach as; the plan is then that of one slice, and
// the fused forms (bn, bnin) exist only at chunks == 1 (bn is not offered, bnin is unsupported)
py::dict conv_plan(int N, int H, int W, int C1, int C2, int Cout, int taps, int packed, int kernel, bool stats,
                   bool eval, int split, long ws_elems, bool pool, bool up, bool bn, bool wfrag, bool bnin) {
  const int Cy1 = split > 0 ? split : Cout;
  const int nc = chunk_images((long)H * W * std::max({C1, C2, Cy1, Cout - Cy1}) * 2, N);
  const int chunks = N > 0 ? (N + nc - 1) / nc : 1;
  RdpConvQuery q;
  q.N = std::min(N, nc); q.H = H; q.W = W; q.C1 = C1; q.C2 = C2; q.Cout = Cout; q.taps = taps; q.packed = packed;
  q.kernel = bnin && chunks > 1 ? RDP_CONV_UNSUPPORTED : kernel;
  q.stats = stats; q.eval = eval; q.split = split; q.ws_elems = ws_elems; q.pool = pool; q.up = up;
  q.bn = bn && chunks == 1; q.bnin = bnin; q.wfrag = wfrag;
  const RdpConvPlan p = rdp_conv_plan_dense(q);
  py::dict d;
  d["kernel"] = p.kernel; d["name"] = rdp_conv_kernel_name(p.kernel); d["chunks"] = chunks;
  d["ring_form"] = p.kernel == RDP_CONV_RING ? p.ring_form : -1;
  d["bm"] = p.BM; d["bn"] = p.BN; d["waves"] = p.waves; d["ksplit"] = p.ksplit; d["rowband_mode"] = p.rowband_mode;
  d["launches"] = p.launches; d["grid"] = p.grid; d["reduce_grid"] = p.rgrid; d["stats_rows"] = p.stats_rows;
  d["ws_elems"] = p.ws_elems; d["pool_fused"] = p.pool_fused; d["up_fused"] = p.up_fused; d["bn_rows"] = p.bn_rows;
  return d;
}

// What conv_fwd and conv_dgrad have validated, for conv_run. The tensors are views (an undefined Act: not given) that
// conv_run binds slice by slice; the blocks carry everything else a launch takes: c the weights, the stats slab and
// the eval epilogue, fuse the upsample's placement, bn the owner layer's coefficients and row slab (dgrad), in the
// producer's BN + ReLU (forward: x1 is its pre-BN output, a_out also receives the activation).
struct ConvCall {
  const char* what = "conv";
  Act x1, x2, y1, y2, pool, up, bn_y, a_out;
  RdpConv c;
  RdpConvFuse fuse;
  RdpConvBnBwd bn;
  RdpConvBnIn in;
  int taps = 9, packed = 0, kernel = RDP_CONV_AUTO;
  long stats_rows = 0, bn_rows = 0;  // what the stats slab / bn.bnpart hold
  float* ws = nullptr;
  long ws_elems = 0;
  const void* wfrag = nullptr;  // (eval) the fragment-major copy of the weights, for the row-band kernel
  long wfrag_bytes = 0;
};
struct ConvRows {
  int stats = 0, bn = 0;  // what the launches reported (the stats-slab rows) / rows written to bn.bnpart
};

// The one bind / chunk / launch body. Batch chunks: the conv kernels address each tensor through ONE buffer
// descriptor with 32-bit offsets (< 2 GiB), so a batch whose largest tensor passes that (256^2 x 64 ch bf16 at
// N >= 256) runs as consecutive launches over image slices (convs never cross images); BN partial rows of the
// slices are appended, fused pool / upsample outputs sliced alike. A chunked batch is offered no BN-backward
// operand (0 rows: the caller's separate pass) and cannot apply a BN to its input.
ConvRows conv_run(const ConvCall& k) {
  const Act &a1 = k.x1, &o1 = k.y1;
  const int Cout = o1.C + k.y2.C, taps = k.taps, packed = k.packed, kernel = k.kernel;
  const int nc = chunk_images({a1, k.x2, o1, k.y2, k.bn_y, k.a_out}, a1.N);
  TORCH_CHECK(!k.in.iscale || nc >= a1.N, k.what, ": in_coef needs a batch that runs as one launch (tensors < 2 GiB)");
  float* const wsp = k.ws;
  const long wsn = k.ws_elems, wfn = k.wfrag_bytes;
  const void* const wfp = k.wfrag;
  const bool want_fused = k.pool.ptr || k.up.ptr;
  ConvRows rows;
  for (int n0 = 0; n0 < a1.N; n0 += nc) {
    const int nn = std::min(nc, a1.N - n0);
    if (k.c.stats)
      TORCH_CHECK(rows.stats + rdp_conv_stats_rows((long)nn * a1.H * a1.W, Cout, kernel) <= k.stats_rows,
                  "stats slab too small");
    // every launch argument is a value here (the blocks are captured by copy): RDP_PLAN may keep the launch for
    // replay (plan mode)
    RdpConv c = k.c;
    conv_bind(c, kX1, a1, n0, nn);
    conv_bind(c, kX2, k.x2, n0, nn);
    conv_bind(c, kY1, o1, n0, nn);
    conv_bind(c, kY2, k.y2, n0, nn);
    if (c.stats) c.stats += (long)rows.stats * 2 * Cout;
    c.Cout = Cout;
    RdpConvFuse fuse = k.fuse;
    if (k.pool.ptr) { fuse.pool = k.pool.image(n0); fuse.ppitch = k.pool.pitch; }
    if (k.up.ptr) { fuse.up = k.up.image(n0); fuse.upitch = k.up.pitch; fuse.uH = k.up.H; fuse.uW = k.up.W; }
    RdpConvBnBwd bn;
    if (k.bn_y.ptr && nc >= a1.N) { bn = k.bn; bn.bny = k.bn_y.ptr; bn.bnypitch = k.bn_y.pitch; }
    RdpConvBnIn in = k.in;
    if (k.a_out.ptr) { in.aout = k.a_out.ptr; in.abytes = k.a_out.bytes; in.apitch = k.a_out.pitch; }
    if (bn.bny)  // the rows the launch below will write
      TORCH_CHECK(rdp_conv_plan(c, taps, packed, kernel, wsp && wsn > 0, wsn, fuse, want_fused, bn, in, wfp ? wfn : 0)
                      .bn_rows <= k.bn_rows, k.what, ": partial too small");
    // the fused pool / upsample flag and the BN-backward row count: heap cells owned by the launch. They are named
    // inside the closure so that a recorded launch owns the cells it writes on every replay
    auto pooled = std::make_shared<int>(0);
    auto bnrows = std::make_shared<int>(0);
    const int r = RDP_PLAN(rdp_conv_igemm(c, taps, packed, kernel, wsp, wsn, wfp, wfn, fuse,
                                          want_fused ? pooled.get() : nullptr, bn, bnrows.get(), in, st));
    TORCH_CHECK(r >= 0, k.what, ": no kernel for this conv (C1=", a1.C, ", C2=", c.C2, ", Cout=", Cout, ", kernel=",
                rdp_conv_kernel_name(kernel), " (", kernel, ")", in.iscale ? ", BN on the input" : "", ")");
    void* const py1 = c.y1;
    const int oH = o1.H, oW = o1.W, oC = o1.C, op1 = o1.pitch;
    if (k.pool.ptr && !*pooled)
      TORCH_CHECK(RDP_PLAN(rdp_maxpool2_fwd(py1, op1, fuse.pool, fuse.ppitch, nn, oH, oW, oC, st)) == 0,
                  "conv_fwd: maxpool");
    if (k.up.ptr && !*pooled)
      TORCH_CHECK(RDP_PLAN(rdp_upsample2_fwd(py1, op1, fuse.up, fuse.upitch, nn, oH, oW, fuse.uH, fuse.uW, fuse.uoy,
                                             fuse.uox, oC, nullptr, st)) == 0,
                  "conv_fwd: upsample");
    rows.stats += r;
    rows.bn += *bnrows;
  }
  return rows;
}

// the sources, destinations, weights and split-K workspace both conv bindings take
void conv_operands(ConvCall& k, const torch::Tensor& x1, const torch::Tensor& w, const torch::Tensor& y1,
                   const c10::optional<torch::Tensor>& y2, const c10::optional<torch::Tensor>& ws) {
  k.x1 = act(x1, "x1");
  k.y1 = act(y1, "y1");
  if (y2) k.y2 = act(*y2, "y2");
  TORCH_CHECK(k.y1.N == k.x1.N && k.y1.H == k.x1.H && k.y1.W == k.x1.W, k.what, ": y spatial mismatch");
  conv_weights(k.c, w);
  TORCH_CHECK(w.size(0) == k.y1.C + k.y2.C, k.what, ": w rows != Cout");
  if (ws) { check_f32(*ws, "ws"); k.ws = ws->data_ptr<float>(); k.ws_elems = ws->numel(); }
}

// y = conv(cat(x1, x2), w); returns #M-tiles (stats rows). in_coef (training, the row ring's 64 -> 64 form only:
// anything else is an error): x1 is the producer layer's PRE-BN output and the conv applies that layer's BN + ReLU
// (in_coef: its [mean|invstd|scale|shift]) to the rows it stages, so the activation need not exist; a_out: it is
// also written there, bitwise what bn_relu_apply writes, for a plain weight-gradient pass.
int conv_fwd(torch::Tensor x1, c10::optional<torch::Tensor> x2, torch::Tensor w, int taps, int packed,
             torch::Tensor y1, c10::optional<torch::Tensor> y2, c10::optional<torch::Tensor> stats, int bm_pref,
             c10::optional<torch::Tensor> affine, int relu, c10::optional<torch::Tensor> ws,
             c10::optional<torch::Tensor> pool, c10::optional<torch::Tensor> up, int up_oy, int up_ox,
             c10::optional<torch::Tensor> wfrag, c10::optional<torch::Tensor> in_coef,
             c10::optional<torch::Tensor> a_out) {
  ConvCall k;
  k.what = "conv_fwd";
  conv_operands(k, x1, w, y1, y2, ws);
  const Act &a1 = k.x1, &o1 = k.y1;
  if (x2) {
    k.x2 = act(*x2, "x2");
    TORCH_CHECK(k.x2.N == a1.N && k.x2.H == a1.H && k.x2.W == a1.W, "x2 spatial mismatch");
  }
  k.taps = taps; k.packed = packed; k.kernel = bm_pref; k.c.erelu = relu;
  const int Cout = o1.C + k.y2.C;
  if (stats) {
    check_f32(*stats, "stats");
    const long rows = rdp_conv_stats_rows((long)a1.N * a1.H * a1.W, Cout, bm_pref);
    TORCH_CHECK(stats->numel() >= rows * 2 * Cout, "stats slab too small");
    k.c.stats = stats->data_ptr<float>();
    k.stats_rows = stats->numel() / (2l * Cout);
  }
  if (affine) {  // BN coefficient block (bn_dev.h layout, BN_ROWS * Cout floats)
    check_f32(*affine, "affine");
    TORCH_CHECK(affine->numel() >= (long)BN_ROWS * Cout, "affine must hold 4*Cout floats");
    k.c.escale = affine->data_ptr<float>() + bn_off(BN_SCALE, Cout);
    k.c.eshift = affine->data_ptr<float>() + bn_off(BN_SHIFT, Cout);
  }
  // pool (eval): MaxPool2d(2) of y1 -> pool [N][H/2][W/2][Cout]; fused into the split-K reduce when
  // that path runs, else a maxpool2_fwd launch after the conv
  if (pool) {
    const Act& po = k.pool = act(*pool, "pool");
    TORCH_CHECK(!y2 && !stats && po.N == o1.N && po.H == o1.H / 2 && po.W == o1.W / 2 && po.C == o1.C,
                "pool: eval conv with one destination, [N][H/2][W/2][Cout]");
  }
  // up (eval): bilinear x2 upsample of y1 into up at (up_oy, up_ox); fused into the split-K reduce
  // when that path runs, else an upsample2_fwd launch after the conv
  if (up) {
    const Act& uo = k.up = act(*up, "up");
    TORCH_CHECK(!pool && !y2 && !stats && uo.N == o1.N && uo.C == o1.C && up_oy >= 0 && up_ox >= 0 &&
                2 * o1.H + up_oy <= uo.H && 2 * o1.W + up_ox <= uo.W, "up: eval conv, [N][>=2H][>=2W][Cout]");
    k.fuse.uoy = up_oy; k.fuse.uox = up_ox;
  }
  if (wfrag) { k.wfrag = wfrag->data_ptr(); k.wfrag_bytes = (long)wfrag->numel() * 2; }
  if (in_coef) {
    check_f32(*in_coef, "in_coef");
    TORCH_CHECK(in_coef->numel() >= (long)BN_ROWS * a1.C, "in_coef: [4 C] f32");
    k.in.iscale = in_coef->data_ptr<float>() + bn_off(BN_SCALE, a1.C);
    k.in.ishift = in_coef->data_ptr<float>() + bn_off(BN_SHIFT, a1.C);
  }
  if (a_out && a_out->defined()) {
    const Act& q = k.a_out = act(*a_out, "a_out");
    TORCH_CHECK(in_coef && q.N == a1.N && q.H == a1.H && q.W == a1.W && q.C == a1.C, "a_out: with in_coef, x1's shape");
  }
  return conv_run(k).stats;
}

// The input gradient dx1 | dx2 = conv(dy, w), w the dgrad weights [Cin][taps * Cout], split over the concat's two
// sources. bn_y / bn_coef / bn_partial (together, one destination): dx1 is the activation gradient of one BN + ReLU
// layer (bn_y: its pre-BN output, bn_coef: its [mean|invstd|scale|shift]), and where the kernel that runs can --
// the row ring's epilogue, the split-K reduce -- it also writes that layer's BN-backward partial rows to
// bn_partial. Returns their count for bn_bwd_finalize; 0: none written, the caller runs bn_relu_bwd_reduce. The
// dgrad always runs.
int conv_dgrad(torch::Tensor dy, torch::Tensor w, torch::Tensor dx1, c10::optional<torch::Tensor> dx2,
               c10::optional<torch::Tensor> ws, c10::optional<torch::Tensor> bn_y, c10::optional<torch::Tensor> bn_coef,
               c10::optional<torch::Tensor> bn_partial, int kernel) {
  ConvCall k;
  k.what = "conv_dgrad";
  conv_operands(k, dy, w, dx1, dx2, ws);
  const Act &a = k.x1, &o = k.y1;
  TORCH_CHECK(w.size(1) % a.C == 0, "conv_dgrad: w must be [Cin][taps * Cout]");
  k.taps = (int)(w.size(1) / a.C); k.kernel = kernel;
  if (bn_y || bn_coef || bn_partial) {
    TORCH_CHECK(bn_y && bn_coef && bn_partial && !dx2, "conv_dgrad: bn_y, bn_coef, bn_partial go together, with one dx");
    const Act& b = k.bn_y = act(*bn_y, "bn_y");
    TORCH_CHECK(b.N == a.N && b.H == a.H && b.W == a.W && b.C == o.C, "conv_dgrad: bn_y shape mismatch");
    check_f32(*bn_coef, "bn_coef");
    check_f32(*bn_partial, "bn_partial");
    TORCH_CHECK(bn_coef->numel() >= (long)BN_ROWS * o.C, "bn_coef must hold 4*C floats");
    k.bn.bncoef = bn_coef->data_ptr<float>();
    k.bn.bnpart = bn_partial->data_ptr<float>();
    k.bn_rows = bn_partial->numel() / (2l * o.C);
  }
  return conv_run(k).bn;
}


// The sources and dy of a weight-gradient operand block = images [n0, n0 + nn) of the tensors (an undefined Act
// leaves its slot empty); x1 sets N / H / W, dy the output channels
void wgrad_bind(RdpWgrad& g, const Act& x1, const Act& x2, const Act& dy, int n0, int nn) {
  g.x1 = x1.image(n0); g.xbytes1 = x1.span_bytes(nn); g.C1 = x1.C; g.pitch1 = x1.pitch;
  if (x2.ptr) { g.x2 = x2.image(n0); g.xbytes2 = x2.span_bytes(nn); g.C2 = x2.C; g.pitch2 = x2.pitch; }
  if (dy.ptr) { g.dy = dy.image(n0); g.dybytes = dy.span_bytes(nn); g.dypitch = dy.pitch; g.Cout = dy.C; }
  g.N = nn; g.H = x1.H; g.W = x1.W;
}

// the fp32 slab and the gradient a weight-gradient launch writes
void wgrad_dest(RdpWgrad& g, const torch::Tensor& slab, const torch::Tensor& out, int accumulate) {
  check_f32(slab, "slab");
  check_f32(out, "out");
  g.slab = slab.data_ptr<float>(); g.slab_elems = slab.numel();
  g.out = out.data_ptr<float>(); g.accumulate = accumulate;
}

int conv_wgrad(torch::Tensor x1, c10::optional<torch::Tensor> x2, torch::Tensor dy, int taps, int packed, int cin_real,
               torch::Tensor slab, torch::Tensor out, int accumulate, int splits, int variant) {
  Act a1 = act(x1, "x1"), a2;
  if (x2) a2 = act(*x2, "x2");
  Act d = act(dy, "dy");
  TORCH_CHECK(d.N == a1.N && d.H == a1.H && d.W == a1.W, "dy spatial mismatch");
  TORCH_CHECK(variant == RDP_WGRAD_AUTO || variant == RDP_WGRAD_GENERIC || variant == RDP_WGRAD_HALO,
              "conv_wgrad: variant must be WGRAD_AUTO, WGRAD_GENERIC or WGRAD_HALO, not ", variant);
  RdpWgrad g;
  wgrad_dest(g, slab, out, accumulate);
  g.taps = taps; g.packed = packed; g.cin_real = cin_real;
  const int Cin = packed ? cin_real : a1.C + a2.C;
  TORCH_CHECK(out.numel() == (long)d.C * taps * Cin, "wgrad out numel mismatch");
  // batch chunks below the 2 GiB buffer-offset reach (see conv_fwd), accumulated into out
  const int nc = chunk_images({a1, a2, d}, a1.N);
  int r = 0;
  for (int n0 = 0; n0 < a1.N; n0 += nc) {
    wgrad_bind(g, a1, a2, d, n0, std::min(nc, a1.N - n0));
    if (n0 > 0) g.accumulate = 1;
    r = RDP_PLAN(rdp_conv_wgrad(g, variant, splits, st));
    TORCH_CHECK(r >= 0, "conv_wgrad: unsupported shape or slab too small (code ", r, ")");
  }
  return r;
}

// First layer: BN-backward apply (+ ReLU mask) fused into the packed weight gradient (conv_wgrad.hip).
// x: the 8-channel packed input, da: dL/d(post-ReLU activation), y: pre-BN conv output, coef / coef2:
// the layer's BN coefficients (bn_finalize / bn_bwd_finalize). Returns the splits, or -1 when the
// shape does not fit the kernel (nothing launched: the caller runs bn_relu_bwd_apply + conv_wgrad).
int wgrad_first_bn(torch::Tensor x, torch::Tensor da, torch::Tensor y, torch::Tensor coef, torch::Tensor coef2,
                   torch::Tensor slab, torch::Tensor out, int cin_real, int accumulate, int splits) {
  Act a = act(x, "x"), d = act(da, "da"), b = act(y, "y");
  TORCH_CHECK(a.C == 8 && d.C == 64 && b.C == 64, "wgrad_first_bn: x must have 8 (packed) and da / y 64 channels");
  TORCH_CHECK(d.N == a.N && d.H == a.H && d.W == a.W && b.N == a.N && b.H == a.H && b.W == a.W,
              "wgrad_first_bn: spatial mismatch");
  check_f32(coef, "coef"); check_f32(coef2, "coef2");
  RdpWgrad g;
  wgrad_dest(g, slab, out, accumulate);
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * 64 && coef2.numel() >= BN2_ROWS * 64, "wgrad_first_bn: coef / coef2 too small");
  TORCH_CHECK(out.numel() == 64l * 9 * cin_real, "wgrad_first_bn: out numel mismatch");
  if (a.bytes >= (1l << 31) || d.bytes >= (1l << 31) || b.bytes >= (1l << 31)) return -1;
  if (((long)a.N * a.H * a.W) % 64) return -1;
  wgrad_bind(g, a, Act{}, Act{}, 0, a.N);
  g.Cout = 64; g.taps = 9; g.packed = 1; g.cin_real = cin_real;
  RdpWgradBn bn;
  bn.da = d.ptr; bn.dabytes = d.bytes; bn.dapitch = d.pitch;
  bn.y = b.ptr; bn.ybytes = b.bytes; bn.ypitch = b.pitch;
  bn.coef = coef.data_ptr<float>(); bn.coef2 = coef2.data_ptr<float>();
  const int r = RDP_PLAN(rdp_wgrad_first_bn(g, bn, splits, st));
  TORCH_CHECK(r > 0, "wgrad_first_bn: slab too small (code ", r, ")");
  return r;
}

// The plan of a dense weight gradient of this shape, as a dict (kernel: the RdpWgradKernel value, -1 = unsupported;
// status: 0, or the RdpWgradStatus the launcher would return). upT: the ConvTranspose2d form (c1 = C, cout = its
// input channels, h / w = the low-res map); first_bn: the first layer's fused form.
py::dict wgrad_plan(int N, int H, int W, int C1, int C2, int Cout, int taps, int packed, int cin_real, int kernel,
                    int splits, long slab_elems, bool upT, bool first_bn) {
  RdpWgradQuery q;
  q.N = N; q.H = H; q.W = W; q.C1 = C1; q.C2 = C2; q.Cout = Cout; q.taps = taps; q.packed = packed;
  q.cin_real = cin_real; q.kernel = kernel; q.splits = splits; q.slab_elems = slab_elems; q.upT = upT;
  q.first_bn = first_bn;
  const RdpWgradPlan p = rdp_wgrad_plan_dense(q);
  py::dict d;
  d["status"] = p.status; d["kernel"] = p.kernel; d["name"] = rdp_wgrad_kernel_name(p.kernel);
  d["bn"] = p.BN; d["multirow"] = p.multirow; d["tiles"] = p.tiles; d["splits"] = p.splits;
  d["per_split"] = p.per_split; d["grid"] = p.grid; d["block"] = p.block; d["slab_elems"] = p.slab_elems;
  d["reduce_groups"] = p.reduce.G; d["reduce_grid1"] = p.reduce.grid1; d["reduce_grid2"] = p.reduce.grid2;
  d["reduce_vec"] = p.reduce.vec;
  return d;
}

void bn_finalize(torch::Tensor stats, int T, long count, torch::Tensor gamma, torch::Tensor beta,
                 c10::optional<torch::Tensor> rmean, c10::optional<torch::Tensor> rvar,
                 c10::optional<torch::Tensor> nbt, double momentum, double eps, torch::Tensor coef,
                 c10::optional<torch::Tensor> ws) {
  const int C = gamma.numel();
  check_f32(stats, "stats"); check_f32(gamma, "gamma"); check_f32(beta, "beta"); check_f32(coef, "coef");
  TORCH_CHECK(stats.numel() >= (long)T * 2 * C && coef.numel() >= (long)BN_ROWS * C, "bn_finalize sizes");
  float* rm = nullptr; float* rv = nullptr; long long* nb = nullptr;
  if (rmean) { check_f32(*rmean, "rmean"); rm = rmean->data_ptr<float>(); }
  if (rvar) { check_f32(*rvar, "rvar"); rv = rvar->data_ptr<float>(); }
  if (nbt) { TORCH_CHECK(nbt->scalar_type() == torch::kInt64 && nbt->is_cuda(), "nbt int64"); nb = (long long*)nbt->data_ptr(); }
  RDP_PLAN(rdp_bn_finalize(stats.data_ptr<float>(), T, C, count, gamma.data_ptr<float>(), beta.data_ptr<float>(), rm, rv, nb,
                  (float)momentum, (float)eps, coef.data_ptr<float>(), ws_ptr(ws, 2 * C), st));
}

void bn_eval_coef(torch::Tensor gamma, torch::Tensor beta, torch::Tensor rmean, torch::Tensor rvar, double eps,
                  torch::Tensor coef) {
  const int C = gamma.numel();
  check_f32(coef, "coef");
  RDP_PLAN(rdp_bn_eval_coef(C, gamma.data_ptr<float>(), beta.data_ptr<float>(), rmean.data_ptr<float>(), rvar.data_ptr<float>(),
                   (float)eps, coef.data_ptr<float>(), st));
}

void bn_relu_apply(torch::Tensor y, torch::Tensor out, torch::Tensor coef, int relu) {
  Act a = act(y, "y"), o = act(out, "out");
  TORCH_CHECK(a.N == o.N && a.H == o.H && a.W == o.W && a.C == o.C, "bn_relu_apply shape");
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * a.C, "coef");
  TORCH_CHECK(RDP_PLAN(rdp_bn_relu_apply(a.ptr, a.pitch, o.ptr, o.pitch, coef.data_ptr<float>(), a.N * a.H * a.W, a.C, relu,
                                st)) == 0, "bn_relu_apply");
}

int bn_relu_bwd_reduce(torch::Tensor da, torch::Tensor y, torch::Tensor coef, int relu, torch::Tensor partial) {
  Act d = act(da, "da"), a = act(y, "y");
  TORCH_CHECK(d.N == a.N && d.H == a.H && d.W == a.W && d.C == a.C, "bn bwd shape");
  check_f32(partial, "partial");
  const int maxb = partial.numel() / (2 * a.C);
  const int T = RDP_PLAN(rdp_bn_relu_bwd_reduce(d.ptr, d.pitch, a.ptr, a.pitch, coef.data_ptr<float>(), a.N * a.H * a.W, a.C,
                                       relu, partial.data_ptr<float>(), maxb, st));
  TORCH_CHECK(T > 0, "bn_relu_bwd_reduce");
  return T;
}

void bn_bwd_finalize(torch::Tensor partial, int T, long count, torch::Tensor gamma, torch::Tensor coef,
                     c10::optional<torch::Tensor> dgamma, c10::optional<torch::Tensor> dbeta, torch::Tensor coef2,
                     c10::optional<torch::Tensor> ws) {
  const int C = gamma.numel();
  RDP_PLAN(rdp_bn_bwd_finalize(partial.data_ptr<float>(), T, C, count, gamma.data_ptr<float>(), coef.data_ptr<float>(),
                      dgamma ? dgamma->data_ptr<float>() : nullptr, dbeta ? dbeta->data_ptr<float>() : nullptr,
                      coef2.data_ptr<float>(), ws_ptr(ws, 2 * C), st));
}

void bn_relu_bwd_apply(torch::Tensor da, torch::Tensor y, torch::Tensor coef, torch::Tensor coef2, torch::Tensor dy,
                       int relu) {
  Act d = act(da, "da"), a = act(y, "y"), o = act(dy, "dy");
  TORCH_CHECK(o.N == a.N && o.H == a.H && o.W == a.W && o.C == a.C, "bn bwd apply shape");
  TORCH_CHECK(RDP_PLAN(rdp_bn_relu_bwd_apply(d.ptr, d.pitch, a.ptr, a.pitch, coef.data_ptr<float>(), coef2.data_ptr<float>(),
                                    o.ptr, o.pitch, a.N * a.H * a.W, a.C, relu, st)) == 0, "bn bwd apply");
}

void maxpool2_fwd(torch::Tensor x, torch::Tensor out) {
  Act a = act(x, "x"), o = act(out, "out");
  TORCH_CHECK(o.N == a.N && o.H == a.H / 2 && o.W == a.W / 2 && o.C == a.C, "maxpool shape");
  TORCH_CHECK(RDP_PLAN(rdp_maxpool2_fwd(a.ptr, a.pitch, o.ptr, o.pitch, a.N, a.H, a.W, a.C, st)) == 0, "maxpool");
}

void maxpool2_bwd(torch::Tensor dp, torch::Tensor x, c10::optional<torch::Tensor> dskip, torch::Tensor dx) {
  Act p = act(dp, "dp"), a = act(x, "x"), o = act(dx, "dx"), s;
  if (dskip) { s = act(*dskip, "dskip"); TORCH_CHECK(s.N == a.N && s.H == a.H && s.W == a.W && s.C == a.C, "dskip shape"); }
  TORCH_CHECK(p.N == a.N && p.H == a.H / 2 && p.W == a.W / 2 && p.C == a.C, "maxpool bwd shape");
  TORCH_CHECK(o.N == a.N && o.H == a.H && o.W == a.W && o.C == a.C, "maxpool bwd dx shape");
  TORCH_CHECK(RDP_PLAN(rdp_maxpool2_bwd(p.ptr, p.pitch, a.ptr, a.pitch, dskip ? s.ptr : nullptr, dskip ? s.pitch : 0, o.ptr,
                               o.pitch, a.N, a.H, a.W, a.C, st)) == 0, "maxpool bwd");
}

// training forward at a Down boundary: a = relu(bn(y)) (skip activation) and its 2x2 max pool, one pass
// out = None: only the pool is written (bf16-exact activation, as if a had been stored and re-read)
void bn_relu_apply_pool(torch::Tensor y, c10::optional<torch::Tensor> out, torch::Tensor pool, torch::Tensor coef) {
  Act a = act(y, "y"), o, p = act(pool, "pool");
  if (out) {
    o = act(*out, "out");
    TORCH_CHECK(a.N == o.N && a.H == o.H && a.W == o.W && a.C == o.C, "bn_relu_apply_pool shape");
  }
  TORCH_CHECK(p.N == a.N && p.H == a.H / 2 && p.W == a.W / 2 && p.C == a.C, "bn_relu_apply_pool pool shape");
  check_f32(coef, "coef");
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * a.C, "coef");
  TORCH_CHECK(RDP_PLAN(rdp_bn_relu_apply_pool(a.ptr, a.pitch, out ? o.ptr : nullptr, out ? o.pitch : 0, p.ptr, p.pitch, coef.data_ptr<float>(), a.N, a.H,
                                     a.W, a.C, st)) == 0, "bn_relu_apply_pool: channels must be 2^k in [8, 2048]");
}

// maxpool backward (+ skip gradient) fused with the BN backward reduction of the pooled layer;
// returns the partial rows written (input T of bn_bwd_finalize)
int maxpool2_bwd_bn_reduce(torch::Tensor dp, torch::Tensor x, c10::optional<torch::Tensor> dskip, torch::Tensor dx,
                           torch::Tensor y, torch::Tensor coef, torch::Tensor partial) {
  Act p = act(dp, "dp"), a = act(x, "x"), o = act(dx, "dx"), yy = act(y, "y"), s;
  if (dskip) { s = act(*dskip, "dskip"); TORCH_CHECK(s.N == a.N && s.H == a.H && s.W == a.W && s.C == a.C, "dskip shape"); }
  TORCH_CHECK(p.N == a.N && p.H == a.H / 2 && p.W == a.W / 2 && p.C == a.C, "maxpool bwd shape");
  TORCH_CHECK(o.N == a.N && o.H == a.H && o.W == a.W && o.C == a.C, "maxpool bwd dx shape");
  TORCH_CHECK(yy.N == a.N && yy.H == a.H && yy.W == a.W && yy.C == a.C, "maxpool bwd y shape");
  check_f32(coef, "coef");
  check_f32(partial, "partial");
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * a.C, "coef");
  const int maxb = partial.numel() / (2 * a.C);
  TORCH_CHECK(maxb >= 1, "partial too small");
  const int T = RDP_PLAN(rdp_maxpool2_bwd_bn_reduce(p.ptr, p.pitch, a.ptr, a.pitch, dskip ? s.ptr : nullptr, dskip ? s.pitch : 0,
                                           o.ptr, o.pitch, yy.ptr, yy.pitch, coef.data_ptr<float>(), a.N, a.H, a.W, a.C,
                                           partial.data_ptr<float>(), maxb, st));
  TORCH_CHECK(T > 0, "maxpool2_bwd_bn_reduce: channels must be 2^k in [8, 2048]");
  return T;
}

// coef (optional, fp32 [4C] = mean|invstd|scale|shift): x is pre-BN; BN + ReLU applied on the fly
void upsample2_fwd(torch::Tensor x, torch::Tensor out, int oy, int ox, c10::optional<torch::Tensor> coef) {
  Act a = act(x, "x"), o = act(out, "out");
  TORCH_CHECK(o.N == a.N && o.C == a.C, "upsample shape");
  TORCH_CHECK(2 * a.H + oy <= o.H && 2 * a.W + ox <= o.W && oy >= 0 && ox >= 0, "upsample fwd placement");
  const float* cp = nullptr;
  if (coef && coef->defined()) {
    TORCH_CHECK(coef->is_cuda() && coef->scalar_type() == torch::kFloat32 && coef->numel() >= (long)BN_ROWS * a.C, "coef [4C] f32");
    cp = coef->data_ptr<float>();
  }
  TORCH_CHECK(RDP_PLAN(rdp_upsample2_fwd(a.ptr, a.pitch, o.ptr, o.pitch, a.N, a.H, a.W, o.H, o.W, oy, ox, a.C, cp,
                                st)) == 0,
              "upsample fwd: channels must be 2^k in [8, 2048], pitches multiples of 8");
}

// y/coef/partial (optional): also accumulate the training-BN backward reduction of dx's BN (dx = da of
// the layer whose pre-BN output is y); returns the partial row count (0 without the fusion)
int upsample2_bwd(torch::Tensor dout, torch::Tensor dx, int oy, int ox, c10::optional<torch::Tensor> y,
                  c10::optional<torch::Tensor> coef, c10::optional<torch::Tensor> partial) {
  Act d = act(dout, "dout"), o = act(dx, "dx"), yy;
  TORCH_CHECK(o.N == d.N && o.C == d.C, "upsample bwd shape");
  TORCH_CHECK(2 * o.H + oy <= d.H && 2 * o.W + ox <= d.W && oy >= 0 && ox >= 0, "upsample bwd placement");
  const float* cf = nullptr;
  float* pp = nullptr;
  int maxb = 0;
  if (y) {
    TORCH_CHECK(coef && partial, "upsample2_bwd: y needs coef and partial");
    yy = act(*y, "y");
    TORCH_CHECK(yy.N == o.N && yy.H == o.H && yy.W == o.W && yy.C == o.C, "upsample bwd y shape");
    check_f32(*coef, "coef");
    check_f32(*partial, "partial");
    TORCH_CHECK(coef->numel() >= (long)BN_ROWS * o.C, "coef");
    maxb = std::min<long>(partial->numel() / (2 * o.C), 4096);
    TORCH_CHECK(maxb >= 1, "partial too small");
    cf = coef->data_ptr<float>();
    pp = partial->data_ptr<float>();
  }
  const int T = RDP_PLAN(rdp_upsample2_bwd(d.ptr, d.pitch, o.ptr, o.pitch, o.N, o.H, o.W, d.H, d.W, oy, ox, o.C,
                                  y ? yy.ptr : nullptr, y ? yy.pitch : 0, cf, pp, maxb, st));
  TORCH_CHECK(T >= 0, "upsample2_bwd: channels must be 2^k in [8, 2048], pitches multiples of 8");
  return T;
}

// ConvTranspose2d(2, s2): yT [N,h,w,4C] (+bias) -> u [N,H2,W2,C] at offset (oy, ox), zero elsewhere
void upT_shuffle(torch::Tensor yT, torch::Tensor bias, torch::Tensor u, int oy, int ox) {
  Act y = act(yT, "yT"), o = act(u, "u");
  check_f32(bias, "bias");
  TORCH_CHECK(y.N == o.N && y.C == 4 * o.C && bias.numel() == o.C, "upT_shuffle shapes");
  TORCH_CHECK(oy >= 0 && ox >= 0 && 2 * y.H + oy <= o.H && 2 * y.W + ox <= o.W, "upT_shuffle placement");
  TORCH_CHECK(RDP_PLAN(rdp_upT_shuffle(y.ptr, y.pitch, bias.data_ptr<float>(), o.ptr, o.pitch, y.N, y.H, y.W, o.H, o.W, oy, ox,
                              o.C, st)) == 0, "upT_shuffle");
}

// the placement of the 2h x 2w window of low-res map `low` at (oy, ox) in `big`
RdpUpT upT_place(const Act& big, const Act& low, int oy, int ox, const char* what) {
  TORCH_CHECK(big.N == low.N && oy >= 0 && ox >= 0 && 2 * low.H + oy <= big.H && 2 * low.W + ox <= big.W, what);
  RdpUpT t;
  t.H2 = big.H; t.W2 = big.W; t.oy = oy; t.ox = ox;
  return t;
}

// host only: whether conv_upT_fwd / conv_upT_dgrad take dense tensors of this shape (else they return -1), the tile
py::dict upT_plan(bool fwd, int N, int h, int w, int Cin, int C, int H2, int W2, int oy, int ox) {
  RdpUpT t;
  t.H2 = H2; t.W2 = W2; t.oy = oy; t.ox = ox;
  const RdpUpTGeo g = rdp_upT_geo_dense(fwd, N, h, w, Cin, C, t);
  py::dict d;
  d["fits"] = g.fits; d["bn"] = g.BN; d["grid"] = g.grid;
  return d;
}

// ConvTranspose2d(2, s2) + bias written straight into u at (oy, ox) by the ping-pong GEMM's epilogue
// (w = the [4C][Cin] forward weight). Returns 0, or -1 when that kernel does not take the shape: the
// caller then runs conv_fwd into yT + upT_shuffle. u's border outside the window is not written.
int conv_upT_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor bias, torch::Tensor u, int oy, int ox) {
  Act a = act(x, "x"), o = act(u, "u");
  check_f32(bias, "bias");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16 && w.is_contiguous() && w.dim() == 2 && w.size(0) == 4 * o.C &&
                  w.size(1) >= a.C, "conv_upT_fwd: w must be bf16 [4C][>= Cin]");
  TORCH_CHECK(a.N == o.N && bias.numel() == o.C, "conv_upT_fwd shapes");
  const RdpUpT t = upT_place(o, a, oy, ox, "conv_upT_fwd placement");
  RdpConv c;
  conv_bind(c, kX1, a, 0, a.N);
  conv_bind(c, kY1, o, 0, a.N);
  conv_weights(c, w);
  c.Cout = 4 * o.C;
  const float* const bp = bias.data_ptr<float>();
  return RDP_PLAN(rdp_conv_upT_fwd(c, t, bp, st));
}

// ConvTranspose2d(2, s2) input gradient dx [N,h,w,Cin] read straight from du (its 4 sub-pixels per
// pixel; wd = the [Cin][4C] dgrad weight) on the ping-pong kernel. Returns 0, or -1 (nothing
// launched) where that kernel does not take the shape: the caller unshuffles and runs the GEMM.
int conv_upT_dgrad(torch::Tensor du, torch::Tensor wd, torch::Tensor dx, int oy, int ox) {
  Act d = act(du, "du"), o = act(dx, "dx");
  TORCH_CHECK(wd.scalar_type() == torch::kBFloat16 && wd.is_contiguous() && wd.dim() == 2 && wd.size(0) == o.C &&
                  wd.size(1) >= 4 * d.C, "conv_upT_dgrad: wd must be bf16 [Cin][>= 4C]");
  const RdpUpT t = upT_place(d, o, oy, ox, "conv_upT_dgrad placement");
  RdpConv c;
  conv_bind(c, kX1, d, 0, d.N);
  conv_bind(c, kY1, o, 0, o.N);
  conv_weights(c, wd);
  c.H = o.H; c.W = o.W; c.Cout = o.C;  // the GEMM runs over the low-res map
  return RDP_PLAN(rdp_conv_upT_dgrad(c, t, st));
}

// ConvTranspose2d(2, s2) weight gradient out [Cin][4C] (+)= from du (4 sub-pixels per pixel of x) and
// its input x [N,h,w,Cin]. Returns the split count (< 0: shape not taken, nothing launched).
int conv_wgrad_upT(torch::Tensor du, torch::Tensor x, int oy, int ox, torch::Tensor slab, torch::Tensor out,
                   int accumulate, int splits) {
  Act d = act(du, "du"), a = act(x, "x");
  RdpWgrad g;
  wgrad_dest(g, slab, out, accumulate);
  TORCH_CHECK(out.numel() == (long)a.C * 4 * d.C, "conv_wgrad_upT out numel");
  const RdpUpT t = upT_place(d, a, oy, ox, "conv_wgrad_upT placement");
  wgrad_bind(g, d, Act{}, a, 0, a.N);
  g.H = a.H; g.W = a.W; g.taps = 4;  // the GEMM runs over the low-res map
  return RDP_PLAN(rdp_conv_wgrad_upT(g, t, splits, st));
}

void upT_unshuffle(torch::Tensor du, torch::Tensor dyT, int oy, int ox) {
  Act d = act(du, "du"), y = act(dyT, "dyT");
  TORCH_CHECK(y.N == d.N && y.C == 4 * d.C, "upT_unshuffle shapes");
  TORCH_CHECK(oy >= 0 && ox >= 0 && 2 * y.H + oy <= d.H && 2 * y.W + ox <= d.W, "upT_unshuffle placement");
  TORCH_CHECK(RDP_PLAN(rdp_upT_unshuffle(d.ptr, d.pitch, y.ptr, y.pitch, y.N, y.H, y.W, d.H, d.W, oy, ox, d.C, st)) == 0,
              "upT_unshuffle");
}

// out[c] (+)= sum over pixels and the `groups` channel blocks of x [N,H,W,groups*C]
void colsum_bf16(torch::Tensor x, int groups, torch::Tensor partial, torch::Tensor out, int accumulate) {
  Act a = act(x, "x");
  check_f32(partial, "partial"); check_f32(out, "out");
  TORCH_CHECK(out.numel() * groups == a.C && partial.numel() >= 1024L * a.C + 64L * out.numel(), "colsum_bf16 sizes");
  TORCH_CHECK(RDP_PLAN(rdp_colsum_bf16(a.ptr, a.pitch, (long)a.N * a.H * a.W, a.C, groups, partial.data_ptr<float>(),
                              out.data_ptr<float>(), accumulate, st)) == 0,
              "colsum_bf16: channels must be a power of two in [8, 2048]");
}

int head_partial_blocks(long M) { return rdp_head_partial_blocks(M); }

// coef (training, optional): `a` is the last conv's pre-BN output y and coef its BN coefficients
// gpart + bnpart (with coef, dice_w == 0): the forward also emits the backward partials
// (gpart [nb][65] head grads, bnpart [nb][128] BN-backward rows; nb = head_partial_blocks(M))
void head_fwd(torch::Tensor a, torch::Tensor w, torch::Tensor b, torch::Tensor target, torch::Tensor logits,
              torch::Tensor partial, torch::Tensor sums, torch::Tensor loss, double dice_w, double dice_eps,
              c10::optional<torch::Tensor> coef, c10::optional<torch::Tensor> gpart,
              c10::optional<torch::Tensor> bnpart, double gscale) {
  Act x = act(a, "a");
  TORCH_CHECK(x.C == 64, "head expects 64 channels");
  const long M = (long)x.N * x.H * x.W;
  TORCH_CHECK(target.numel() == M && logits.numel() == M, "head target/logits numel");
  TORCH_CHECK(partial.numel() >= (long)rdp_head_partial_blocks(M) * 65, "head partial too small");
  const float* cf = nullptr;
  if (coef) {
    TORCH_CHECK(coef->numel() >= (long)BN_ROWS * 64 && coef->scalar_type() == torch::kFloat, "head coef");
    cf = coef->data_ptr<float>();
  }
  float* gp = nullptr;
  float* bp = nullptr;
  if (gpart) {
    const long nb = rdp_head_partial_blocks(M);
    TORCH_CHECK(cf && bnpart && dice_w == 0.0, "head_fwd grad partials need coef, bnpart and dice_w == 0");
    check_f32(*gpart, "gpart");
    check_f32(*bnpart, "bnpart");
    TORCH_CHECK(gpart->numel() >= nb * 65 && bnpart->numel() >= nb * 128, "head_fwd grad partials too small");
    gp = gpart->data_ptr<float>();
    bp = bnpart->data_ptr<float>();
  }
  TORCH_CHECK(RDP_PLAN(rdp_head_fwd(x.ptr, x.pitch, w.data_ptr<float>(), b.data_ptr<float>(), target.data_ptr<float>(),
                           logits.data_ptr<float>(), partial.data_ptr<float>(), sums.data_ptr<float>(),
                           loss.data_ptr<float>(), M, (float)dice_w, (float)dice_eps, cf, gp, bp, (float)gscale,
                           st)) > 0, "head_fwd");
}

void head_grad_finalize(torch::Tensor gpart, long M, torch::Tensor gw, torch::Tensor gb) {
  check_f32(gpart, "gpart");
  TORCH_CHECK(gpart.numel() >= (long)rdp_head_partial_blocks(M) * 65 && gw.numel() == 64 && gb.numel() == 1,
              "head_grad_finalize sizes");
  RDP_PLAN(rdp_head_grad_finalize(gpart.data_ptr<float>(), (int)M, gw.data_ptr<float>(), gb.data_ptr<float>(), st));
}

// coef + bnpart given: BN-fused backward (da not written, returns the BN partial row count);
// otherwise da = d loss / d a is written. Returns the number of partial rows.
int head_bwd(torch::Tensor a, torch::Tensor w, torch::Tensor logits, torch::Tensor target, torch::Tensor sums,
             c10::optional<torch::Tensor> da, torch::Tensor partial, torch::Tensor gw, torch::Tensor gb, double dice_w,
             double dice_eps, double gscale, c10::optional<torch::Tensor> coef, c10::optional<torch::Tensor> bnpart) {
  Act x = act(a, "a");
  const long M = (long)x.N * x.H * x.W;
  TORCH_CHECK(x.C == 64, "head bwd channels");
  TORCH_CHECK(partial.numel() >= (long)rdp_head_partial_blocks(M) * 65, "head partial too small");
  void* dptr = nullptr;
  int dpitch = 0;
  const float* cf = nullptr;
  float* bp = nullptr;
  if (coef) {
    TORCH_CHECK(bnpart && bnpart->numel() >= (long)rdp_head_partial_blocks(M) * 128, "head bnpart too small");
    TORCH_CHECK(coef->numel() >= (long)BN_ROWS * 64 && coef->scalar_type() == torch::kFloat, "head coef");
    cf = coef->data_ptr<float>();
    bp = bnpart->data_ptr<float>();
  } else {
    TORCH_CHECK(da.has_value(), "head_bwd: da required without coef");
    Act d = act(*da, "da");
    TORCH_CHECK(d.C == 64 && (long)d.N * d.H * d.W == M, "head bwd da shape");
    dptr = d.ptr;
    dpitch = d.pitch;
  }
  return RDP_PLAN(rdp_head_bwd(x.ptr, x.pitch, w.data_ptr<float>(), logits.data_ptr<float>(), target.data_ptr<float>(),
                      sums.data_ptr<float>(), dptr, dpitch, partial.data_ptr<float>(), gw.data_ptr<float>(),
                      gb.data_ptr<float>(), M, (float)dice_w, (float)dice_eps, (float)gscale, cf, bp, st));
}

// dy of the last conv from the logits (BN-fused head backward, second pass)
void head_bn_bwd_apply(torch::Tensor y, torch::Tensor w, torch::Tensor logits, torch::Tensor target,
                       torch::Tensor sums, torch::Tensor coef, torch::Tensor coef2, torch::Tensor dy, double dice_w,
                       double dice_eps, double gscale) {
  Act x = act(y, "y"), d = act(dy, "dy");
  const long M = (long)x.N * x.H * x.W;
  TORCH_CHECK(x.C == 64 && d.C == 64 && (long)d.N * d.H * d.W == M, "head_bn_bwd_apply shapes");
  TORCH_CHECK(logits.numel() == M && target.numel() == M, "head_bn_bwd_apply logits/target numel");
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * 64 && coef2.numel() >= BN2_ROWS * 64, "head_bn_bwd_apply coef sizes");
  TORCH_CHECK(RDP_PLAN(rdp_head_bn_bwd_apply(x.ptr, x.pitch, w.data_ptr<float>(), logits.data_ptr<float>(),
                                    target.data_ptr<float>(), sums.data_ptr<float>(), coef.data_ptr<float>(),
                                    coef2.data_ptr<float>(), d.ptr, d.pitch, M, (float)dice_w, (float)dice_eps,
                                    (float)gscale, st)) == 0,
              "head_bn_bwd_apply: pitches must be multiples of 8");
}

// The body of conv_head_mask / conv_headk_mask: the eval conv (64 -> 64, BN fold + ReLU) whose output only the fused
// serving head h reads, on the row ring; false (nothing launched) where that kernel does not apply
bool conv_ring_head(const Act& a, const torch::Tensor& w, const torch::Tensor& coef, RdpRingHead h,
                    const torch::Tensor& mask) {
  check_w(w);
  check_f32(coef, "coef");
  const int Co = (int)w.size(0);
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * Co, "coef size");
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kUInt8 && mask.is_contiguous() &&
              mask.numel() >= (long)a.N * a.H * a.W, "mask: u8 [N*H*W]");
  RdpConv c;
  conv_bind(c, kX1, a, 0, a.N);
  conv_weights(c, w);
  c.Cy1 = 64; c.ypitch1 = 64; c.Cout = Co;
  c.escale = coef.data_ptr<float>() + bn_off(BN_SCALE, Co); c.eshift = coef.data_ptr<float>() + bn_off(BN_SHIFT, Co);
  c.erelu = 1;
  h.mask = mask.data_ptr();
  return RDP_PLAN(rdp_conv_ring_head(c, h, st)) == 0;
}

// eval conv (64 -> 64, BN fold + ReLU) + serving 1x1 head + (logit > thr) in one kernel (row ring);
// returns false (nothing launched) where that kernel does not apply
bool conv_head_mask(torch::Tensor x, torch::Tensor w, torch::Tensor coef, torch::Tensor hw, torch::Tensor hb,
                    double thr, torch::Tensor mask) {
  Act a = act(x, "x");
  check_w(w);
  check_f32(hw, "head_w");
  check_f32(hb, "head_b");
  TORCH_CHECK(hw.numel() == w.size(0) && hb.numel() >= 1, "coef / head sizes");
  RdpRingHead h;
  h.hw = hw.data_ptr<float>(); h.hb = hb.data_ptr<float>(); h.thr = (float)thr;
  return conv_ring_head(a, w, coef, h, mask);
}

// Row-band eval conv called directly (csrc/conv_rowband.hip), with OHWI weights (wfrag = 0) or their
// fragment-major copy (wfrag = 1: [Cout/16][9 Cin/32][64 lanes][8], rowband_frag_weights in Python).
// Returns 1 when the pool was written, 0 when not, < 0 when the kernel does not take the shape.
int conv_rowband(torch::Tensor x1, c10::optional<torch::Tensor> x2, torch::Tensor w, torch::Tensor y,
                 torch::Tensor coef, c10::optional<torch::Tensor> pool, int wfrag) {
  Act a1 = act(x1, "x1"), a2;
  if (x2) a2 = act(*x2, "x2");
  Act o = act(y, "y");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 && w.is_contiguous(), "w: bf16 contiguous");
  check_f32(coef, "coef");
  TORCH_CHECK(coef.numel() >= (long)BN_ROWS * o.C, "coef size");
  Act po;
  if (pool) po = act(*pool, "pool");
  RdpConv c;
  conv_bind(c, kX1, a1, 0, a1.N);
  conv_bind(c, kX2, a2, 0, a1.N);
  conv_bind(c, kY1, o, 0, a1.N);
  c.w = w.data_ptr(); c.wbytes = w.numel() * 2; c.ldw = wfrag ? 0 : (int)w.size(1);
  c.Cout = o.C;
  c.escale = coef.data_ptr<float>() + bn_off(BN_SCALE, o.C); c.eshift = coef.data_ptr<float>() + bn_off(BN_SHIFT, o.C); c.erelu = 1;
  void* const pp = pool ? po.ptr : nullptr;
  const long pb = pool ? po.bytes : 0;
  const int ppit = pool ? po.pitch : 0;
  return (int)RDP_PLAN(rdp_conv_rowband_ex(c, pp, pb, ppit, wfrag, st));
}

// Persistent row-band chain (csrc/conv_rowband.hip): layer 0 reads x, layer l > 0 layer l - 1's output;
// eval BN fold + ReLU per layer (coef = [mean|invstd|scale|shift]). cnt: int32 >= 1 + nl * N * H, err: int32.
bool conv_rowband_chain(torch::Tensor x, std::vector<torch::Tensor> ws, std::vector<torch::Tensor> ys,
                        std::vector<torch::Tensor> coefs, torch::Tensor cnt, torch::Tensor err) {
  const int nl = (int)ws.size();
  TORCH_CHECK(nl >= 1 && nl <= 4 && (int)ys.size() == nl && (int)coefs.size() == nl, "1..4 layers");
  Act a = act(x, "x");
  TORCH_CHECK(cnt.is_cuda() && cnt.scalar_type() == torch::kInt32 && cnt.numel() >= 1 + (long)nl * a.N * a.H, "cnt");
  TORCH_CHECK(err.is_cuda() && err.scalar_type() == torch::kInt32 && err.numel() >= 1, "err");
  std::array<const void*, 4> wp{};
  std::array<void*, 4> yp{};
  std::array<long, 4> wb{}, yb{};
  std::array<int, 4> ldw{}, ypit{}, co{};
  std::array<const float*, 4> sc{}, sh{};
  for (int l = 0; l < nl; ++l) {
    TORCH_CHECK(ws[l].is_cuda() && ws[l].scalar_type() == torch::kBFloat16 && ws[l].is_contiguous() && ws[l].dim() == 2,
                "w: bf16 [Cout][K]");
    Act o = act(ys[l], "y");
    TORCH_CHECK(o.N == a.N && o.H == a.H && o.W == a.W && o.C == ws[l].size(0), "y shape");
    check_f32(coefs[l], "coef");
    TORCH_CHECK(coefs[l].numel() >= (long)BN_ROWS * o.C, "coef size");
    wp[l] = ws[l].data_ptr(); wb[l] = ws[l].numel() * 2; ldw[l] = (int)ws[l].size(1);
    yp[l] = o.ptr; yb[l] = o.bytes; ypit[l] = o.pitch; co[l] = o.C;
    sc[l] = coefs[l].data_ptr<float>() + bn_off(BN_SCALE, o.C); sh[l] = coefs[l].data_ptr<float>() + bn_off(BN_SHIFT, o.C);
  }
  int* const cp = cnt.data_ptr<int>();
  int* const ep = err.data_ptr<int>();
  const int r = RDP_PLAN(rdp_conv_rowband_chain(nl, a.ptr, a.bytes, a.C, a.pitch, wp.data(), wb.data(), ldw.data(),
                                                yp.data(), yb.data(), ypit.data(), co.data(), sc.data(), sh.data(),
                                                a.N, a.H, a.W, cp, ep, st));
  return r == 0;
}

void head_mask(torch::Tensor a, torch::Tensor w, torch::Tensor b, double logit_thr, torch::Tensor mask) {
  Act x = act(a, "a");
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8 && mask.numel() == (long)x.N * x.H * x.W, "mask u8 numel");
  RDP_PLAN(rdp_head_mask(x.ptr, x.pitch, w.data_ptr<float>(), b.data_ptr<float>(), (float)logit_thr, mask.data_ptr(),
                x.N * x.H * x.W, st));
}

// ---- K-class head (csrc/head_multi.hip): w [K][64] fp32 (outc.conv.weight's physical layout), b [K] ----
int headk_partial_blocks(long M) { return rdp_headk_partial_blocks(M); }

// the class count of a K-class head call, from its weight / bias operands (2 <= K <= 8)
int headk_classes(const torch::Tensor& w, const torch::Tensor& b, const char* who) {
  check_f32(w, "w");
  check_f32(b, "b");
  const long K = b.numel();
  TORCH_CHECK(K >= 2 && K <= 8, who, ": the K-class head takes 2 <= K <= 8 classes, got ", K);
  TORCH_CHECK(w.numel() == K * 64, who, ": w must be [K][64]");
  return (int)K;
}

void check_u8(const torch::Tensor& t, long numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kUInt8 && t.is_contiguous() && t.numel() == numel, name,
              ": must be a contiguous u8 GPU tensor of ", numel, " elements");
}

// The optional extended mode of the K-class head: class weights (fp32 [K] on the device; their VALUES are the
// caller's to validate, nothing here syncs) and / or a soft Dice term. Returns the weights' pointer (null: none);
// `ext` = the call runs the extended kernels, which need 2 + 3K floats of `sums`.
const float* headk_ext_args(const c10::optional<torch::Tensor>& class_weights, double dice_w, double dice_eps, int K,
                            const torch::Tensor& sums, const char* who, bool& ext) {
  TORCH_CHECK(dice_w >= 0.0 && std::isfinite(dice_w), who, ": dice_w must be finite and >= 0, got ", dice_w);
  TORCH_CHECK(dice_eps > 0.0 && std::isfinite(dice_eps), who, ": dice_eps must be finite and > 0, got ", dice_eps);
  const float* cw = nullptr;
  if (class_weights) {
    const torch::Tensor& t = *class_weights;
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() == K, who,
                ": class_weights must be a contiguous fp32 GPU tensor of ", K, " elements");
    cw = t.data_ptr<float>();
  }
  ext = cw != nullptr || (float)dice_w != 0.f;
  TORCH_CHECK(!ext || sums.numel() >= 2 + 3 * K, who, ": class weights / Dice need 2 + 3K = ", 2 + 3 * K,
              " floats of sums, got ", sums.numel());
  return cw;
}

// logits [M][K] fp32, softmax cross-entropy over the labels < K (u8; 255 and every label >= K ignored):
// loss[0] = loss[1] = mean over the kept pixels, sums[0..1] = {sum ce, kept pixels}. With class_weights and / or
// dice_w > 0: loss[0] = CE + dice_w * Dice, loss[1] = the weighted CE, sums[0 .. 2+3K) = {sum w*ce, W, I_k, P_k, T_k}
void headk_fwd(torch::Tensor a, torch::Tensor w, torch::Tensor b, torch::Tensor labels, torch::Tensor logits,
               torch::Tensor partial, torch::Tensor sums, torch::Tensor loss,
               c10::optional<torch::Tensor> class_weights, double dice_w, double dice_eps) {
  Act x = act(a, "a");
  const int K = headk_classes(w, b, "headk_fwd");
  TORCH_CHECK(x.C == 64, "head expects 64 channels");
  const long M = (long)x.N * x.H * x.W;
  TORCH_CHECK(M > 0 && M < (1L << 31), "headk_fwd: pixel count");
  check_u8(labels, M, "labels");
  check_f32(logits, "logits");
  check_f32(partial, "partial");
  check_f32(sums, "sums");
  check_f32(loss, "loss");
  bool ext = false;
  const float* cw = headk_ext_args(class_weights, dice_w, dice_eps, K, sums, "headk_fwd", ext);
  TORCH_CHECK(logits.numel() == M * K, "headk_fwd: logits must hold M * K values");
  TORCH_CHECK(partial.numel() >= (long)rdp_headk_partial_blocks(M) * (ext ? 2 + 3 * K : 2),
              "headk_fwd: partial too small");
  TORCH_CHECK(sums.numel() >= 2 && loss.numel() >= 2, "headk_fwd: sums / loss need 2 values");
  TORCH_CHECK(RDP_PLAN(rdp_headk_fwd(x.ptr, x.pitch, w.data_ptr<float>(), b.data_ptr<float>(), labels.data_ptr(),
                                     logits.data_ptr<float>(), partial.data_ptr<float>(), sums.data_ptr<float>(),
                                     loss.data_ptr<float>(), (int)M, K, cw, (float)dice_w, (float)dice_eps, st)) > 0,
              "headk_fwd");
}

// da = d loss / d a (bf16), gw [K][64] / gb [K] = the head's gradients; partial: >= blocks * (K * 65) floats.
// class_weights / dice_w / dice_eps: as given to headk_fwd, whose `sums` this reads.
void headk_bwd(torch::Tensor a, torch::Tensor w, torch::Tensor logits, torch::Tensor labels, torch::Tensor sums,
               torch::Tensor da, torch::Tensor partial, torch::Tensor gw, torch::Tensor gb, double gscale,
               c10::optional<torch::Tensor> class_weights, double dice_w, double dice_eps) {
  Act x = act(a, "a"), d = act(da, "da");
  const int K = headk_classes(w, gb, "headk_bwd");
  const long M = (long)x.N * x.H * x.W;
  TORCH_CHECK(M > 0 && M < (1L << 31), "headk_bwd: pixel count");
  TORCH_CHECK(x.C == 64 && d.C == 64 && (long)d.N * d.H * d.W == M, "headk_bwd: a / da shapes");
  check_u8(labels, M, "labels");
  check_f32(logits, "logits");
  check_f32(partial, "partial");
  check_f32(sums, "sums");
  check_f32(gw, "gw");
  bool ext = false;
  const float* cw = headk_ext_args(class_weights, dice_w, dice_eps, K, sums, "headk_bwd", ext);
  TORCH_CHECK(logits.numel() == M * K && sums.numel() >= 2 && gw.numel() == K * 64, "headk_bwd: logits / sums / gw sizes");
  TORCH_CHECK(partial.numel() >= (long)rdp_headk_partial_blocks(M) * (K * 65), "headk_bwd: partial too small");
  TORCH_CHECK(RDP_PLAN(rdp_headk_bwd(x.ptr, x.pitch, w.data_ptr<float>(), logits.data_ptr<float>(), labels.data_ptr(),
                                     sums.data_ptr<float>(), d.ptr, d.pitch, partial.data_ptr<float>(),
                                     gw.data_ptr<float>(), gb.data_ptr<float>(), (int)M, K, (float)gscale, cw,
                                     (float)dice_w, (float)dice_eps, st)) > 0,
              "headk_bwd");
}

// serving: mask[p] = (argmax_k logits[p][k] == cls), ties to the lowest class
void headk_mask(torch::Tensor a, torch::Tensor w, torch::Tensor b, int cls, torch::Tensor mask) {
  Act x = act(a, "a");
  const int K = headk_classes(w, b, "headk_mask");
  TORCH_CHECK(x.C == 64, "head expects 64 channels");
  const long M = (long)x.N * x.H * x.W;
  TORCH_CHECK(M > 0 && M < (1L << 31), "headk_mask: pixel count");
  TORCH_CHECK(cls >= 0 && cls < K, "headk_mask: class ", cls, " outside 0..", K - 1);
  check_u8(mask, M, "mask");
  TORCH_CHECK(RDP_PLAN(rdp_headk_mask(x.ptr, x.pitch, w.data_ptr<float>(), b.data_ptr<float>(), cls, mask.data_ptr(),
                                      (int)M, K, st)) == 0, "headk_mask");
}

// conv_head_mask with the K-class head (head_w [K*64], head_b [K], 2 <= K <= 8): mask = (arg-max class == cls, ties to
// the lowest class), bit for bit conv_fwd + headk_mask; returns false (nothing launched) where the ring kernel
// does not apply
bool conv_headk_mask(torch::Tensor x, torch::Tensor w, torch::Tensor coef, torch::Tensor hw, torch::Tensor hb, int cls,
                     torch::Tensor mask) {
  Act a = act(x, "x");
  RdpRingHead h;
  h.K = headk_classes(hw, hb, "conv_headk_mask");
  TORCH_CHECK(cls >= 0 && cls < h.K, "conv_headk_mask: class ", cls, " outside 0..", h.K - 1);
  const long M = (long)a.N * a.H * a.W;
  TORCH_CHECK(M > 0 && M < (1L << 31), "conv_headk_mask: pixel count");
  h.hw = hw.data_ptr<float>(); h.hb = hb.data_ptr<float>(); h.cls = cls;
  return conv_ring_head(a, w, coef, h, mask);
}

// ---- validation metrics (csrc/seg_metrics.hip) ----
int seg_confusion_blocks(long M) { return rdp_seg_confusion_blocks(M); }
int seg_confusion_block_pixels() { return rdp_seg_confusion_block_pixels(); }

// counts (int64 [KC * KC + 1], KC = max(K, 2)) += the confusion counts of `logits` against `target`:
// K >= 2: logits fp32 [M * K] pixel-major, target u8 [M], arg-max with ties to the lowest class, labels >= K
// ignored (last slot); K == 1: logits fp32 [M], target fp32 [M], logit > thr against target > 0.5.
// `max_blocks` > 0 caps the grid (tests: a small M then takes several passes of the grid-stride loop).
void seg_confusion(torch::Tensor logits, torch::Tensor target, int K, torch::Tensor counts, double thr,
                   int max_blocks) {
  TORCH_CHECK(K >= 1 && K <= 8, "seg_confusion: 1 <= K <= 8 classes, got ", K);
  TORCH_CHECK(max_blocks >= 0, "seg_confusion: max_blocks");
  check_f32(logits, "logits");
  const long M = target.numel();
  TORCH_CHECK(M > 0 && M < (1L << 31), "seg_confusion: pixel count");
  TORCH_CHECK(logits.numel() == M * K, "seg_confusion: logits must hold M * K values");
  TORCH_CHECK((uintptr_t)logits.data_ptr() % 16 == 0, "seg_confusion: logits must be 16-byte aligned");
  if (K == 1) check_f32(target, "target");
  else check_u8(target, M, "target");
  const int KC = K < 2 ? 2 : K;
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == torch::kInt64 && counts.is_contiguous() &&
                  counts.numel() == (long)KC * KC + 1,
              "seg_confusion: counts must be a contiguous int64 GPU tensor of ", KC * KC + 1, " elements");
  TORCH_CHECK(RDP_PLAN(rdp_seg_confusion(logits.data_ptr<float>(), target.data_ptr(), counts.data_ptr(), M, K,
                                         (float)thr, max_blocks, st)) > 0, "seg_confusion");
}

void adam(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> shadow,
          double lr, double b1, double b2, double eps, double wd, double gscale, torch::Tensor step, bool inc,
          int max_blocks) {
  check_f32(p, "p"); check_f32(m, "m"); check_f32(v, "v");
  const bool gbf = g.scalar_type() == torch::kBFloat16;  // bf16 gradients (the DDP bf16 all-reduce buffer)
  if (!gbf) check_f32(g, "g");
  TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "g: contiguous device tensor");
  TORCH_CHECK(g.numel() == p.numel() && m.numel() == p.numel() && v.numel() == p.numel(), "adam numel");
  TORCH_CHECK(step.scalar_type() == torch::kInt32 && step.is_cuda(), "step int32");
  void* sh = nullptr;
  if (shadow) {
    TORCH_CHECK(shadow->scalar_type() == torch::kBFloat16 && shadow->numel() == p.numel(), "shadow");
    sh = shadow->data_ptr();
  }
  const void* gp = g.data_ptr();
  TORCH_CHECK(RDP_PLAN(rdp_adam(p.data_ptr<float>(), gp, gbf ? 1 : 0, m.data_ptr<float>(), v.data_ptr<float>(), sh, p.numel(),
                       (float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (float)gscale,
                       (int*)step.data_ptr(), inc ? 1 : 0, max_blocks, st)) == 0, "adam: numel must be a multiple of 4");
}

// ---- optimizer scalars on the device: gradient norm, clip coefficient, learning-rate multiplier ----
int grad_sqnorm_blocks(long n) {
  TORCH_CHECK(n > 0 && n % 4 == 0, "grad_sqnorm_blocks: n must be a positive multiple of 4");
  return rdp_grad_sqnorm_blocks(n);
}

// partial[0 .. blocks) = per-block fp64 sums of g^2 (g fp32 or bf16); returns blocks
int grad_sqnorm(torch::Tensor g, torch::Tensor partial, int max_blocks) {
  const bool gbf = g.scalar_type() == torch::kBFloat16;
  if (!gbf) check_f32(g, "g");
  TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "g: contiguous device tensor");
  const long n = g.numel();
  TORCH_CHECK(n > 0 && n % 4 == 0, "grad_sqnorm: numel must be a positive multiple of 4");
  TORCH_CHECK((uintptr_t)g.data_ptr() % (gbf ? 8 : 16) == 0, "grad_sqnorm: g must be aligned to 4 elements");
  TORCH_CHECK(max_blocks >= 0, "grad_sqnorm: max_blocks");
  int blocks = rdp_grad_sqnorm_blocks(n);
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat64 && partial.is_contiguous() &&
                  partial.device() == g.device() && partial.numel() >= blocks,
              "grad_sqnorm: partial must be a contiguous float64 tensor on g's device with at least ", blocks,
              " elements");
  const void* gp = g.data_ptr();
  const int r = RDP_PLAN(rdp_grad_sqnorm(gp, gbf ? 1 : 0, n, partial.data_ptr<double>(), max_blocks, st));
  TORCH_CHECK(r == blocks, "grad_sqnorm");
  return r;
}

void optim_ctl(torch::Tensor partial, int nblocks, double gscale, double clip, int sched, int warmup, int total,
               double min_ratio, torch::Tensor step, torch::Tensor ctl) {
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == torch::kFloat64 && partial.is_contiguous(),
              "optim_ctl: partial must be a contiguous float64 device tensor");
  TORCH_CHECK(nblocks >= 0 && nblocks <= partial.numel(), "optim_ctl: nblocks exceeds the partial buffer");
  TORCH_CHECK(step.scalar_type() == torch::kInt32 && step.is_cuda() && step.numel() >= 1, "step int32");
  check_f32(ctl, "ctl");
  TORCH_CHECK(ctl.numel() >= 4, "optim_ctl: ctl holds 4 floats");
  TORCH_CHECK(std::isfinite(clip) && clip >= 0.0 && std::isfinite(gscale), "optim_ctl: clip / gscale");
  TORCH_CHECK(sched == 0 || sched == 1, "optim_ctl: sched 0 (constant) or 1 (cosine)");
  TORCH_CHECK(warmup >= 0 && min_ratio >= 0.0 && min_ratio <= 1.0, "optim_ctl: warmup / min_ratio");
  TORCH_CHECK(sched == 0 || total > warmup, "optim_ctl: cosine needs total > warmup");
  TORCH_CHECK(RDP_PLAN(rdp_optim_ctl(partial.data_ptr<double>(), nblocks, gscale, clip, sched, warmup, total, min_ratio,
                                     (const int*)step.data_ptr(), ctl.data_ptr<float>(), st)) == 0,
              "optim_ctl: bad argument");
}

void adam_ctl(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> shadow,
              double lr, double b1, double b2, double eps, double wd, double gscale, torch::Tensor step,
              torch::Tensor ctl, bool inc, int max_blocks) {
  check_f32(p, "p"); check_f32(m, "m"); check_f32(v, "v");
  const bool gbf = g.scalar_type() == torch::kBFloat16;  // bf16 gradients (the DDP bf16 all-reduce buffer)
  if (!gbf) check_f32(g, "g");
  TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "g: contiguous device tensor");
  TORCH_CHECK(g.numel() == p.numel() && m.numel() == p.numel() && v.numel() == p.numel(), "adam numel");
  TORCH_CHECK(step.scalar_type() == torch::kInt32 && step.is_cuda(), "step int32");
  check_f32(ctl, "ctl");
  TORCH_CHECK(ctl.numel() >= 4, "adam_ctl: ctl holds 4 floats");
  void* sh = nullptr;
  if (shadow) {
    TORCH_CHECK(shadow->scalar_type() == torch::kBFloat16 && shadow->numel() == p.numel(), "shadow");
    sh = shadow->data_ptr();
  }
  const void* gp = g.data_ptr();
  TORCH_CHECK(RDP_PLAN(rdp_adam_ctl(p.data_ptr<float>(), gp, gbf ? 1 : 0, m.data_ptr<float>(), v.data_ptr<float>(), sh,
                                    p.numel(), (float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (float)gscale,
                                    (int*)step.data_ptr(), ctl.data_ptr<float>(), inc ? 1 : 0, max_blocks, st)) == 0,
              "adam_ctl: numel must be a multiple of 4");
}

void cast_bf16(torch::Tensor p, torch::Tensor out) {
  check_f32(p, "p");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 && out.numel() == p.numel(), "cast out");
  RDP_PLAN(rdp_cast_bf16(p.data_ptr<float>(), out.data_ptr(), p.numel(), st));
}

// The serving runtime's frame upload kernel (csrc/serve_kernels.hip), for tests: a pinned CPU tensor ->
// a device tensor of the same byte size through the host buffer's device mapping. Returns 0, or -1 when
// the kernel does not take the pair (unaligned) or the buffer has no mapping.
int h2d_copy(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(!src.is_cuda() && src.is_pinned() && src.is_contiguous(), "h2d_copy: src must be a pinned CPU tensor");
  TORCH_CHECK(dst.is_cuda() && dst.is_contiguous(), "h2d_copy: dst must be a contiguous device tensor");
  const long bytes = (long)(src.numel() * src.element_size());
  TORCH_CHECK(bytes == (long)(dst.numel() * dst.element_size()), "h2d_copy: byte sizes differ");
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, src.data_ptr(), 0) != hipSuccess || !dp) {
    (void)hipGetLastError();
    return -1;
  }
  return rdp_h2d_copy(dp, dst.data_ptr(), bytes, c10::hip::getCurrentHIPStream().stream());
}

void wprep(torch::Tensor master, torch::Tensor out, torch::Tensor segs, int nseg, c10::optional<torch::Tensor> step,
           int blocks) {
  check_f32(master, "master");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16, "wprep out bf16");
  TORCH_CHECK(segs.is_cuda() && segs.numel() * segs.element_size() >= (long)nseg * rdp_wseg_size(), "segs");
  int* sp = nullptr;
  if (step) {
    TORCH_CHECK(step->scalar_type() == torch::kInt32 && step->is_cuda(), "step int32");
    sp = (int*)step->data_ptr();
  }
  RDP_PLAN(rdp_wprep(master.data_ptr<float>(), out.data_ptr(), segs.data_ptr(), nseg, sp, blocks, 0, st));
}

void check_cpu_f64(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.device().is_cpu() && t.scalar_type() == torch::kFloat64 && t.is_contiguous(), name,
              ": must be a contiguous float64 CPU tensor");
}

// FITPACK parcur: returns (ier, t[n], c[idim][n-k-1], fp)
py::tuple parcur(torch::Tensor u, torch::Tensor x, double s, int k) {
  check_cpu_f64(u, "u"); check_cpu_f64(x, "x");
  const int m = u.numel(), idim = x.size(1);
  TORCH_CHECK(x.size(0) == m, "x rows != len(u)");
  const int nest = m + 2 * k;
  auto t = torch::zeros({nest}, torch::kFloat64), c = torch::zeros({idim, nest}, torch::kFloat64);
  int n = 0;
  double fp = 0;
  int ier;
  {
    py::gil_scoped_release nogil;
    ier = rdp_parcur(idim, m, u.data_ptr<double>(), x.data_ptr<double>(), s, k, nest, t.data_ptr<double>(),
                     c.data_ptr<double>(), &n, &fp);
  }
  if (ier == 10) return py::make_tuple(ier, torch::Tensor(), torch::Tensor(), fp);
  return py::make_tuple(ier, t.narrow(0, 0, n).clone(), c.narrow(1, 0, n - k - 1).clone(), fp);
}

torch::Tensor splev(torch::Tensor t, torch::Tensor c, int k, torch::Tensor x, int der) {
  check_cpu_f64(t, "t"); check_cpu_f64(x, "x");
  auto cc = c.contiguous().to(torch::kFloat64);
  auto out = torch::empty_like(x);
  for (long i = 0; i < x.numel(); ++i)
    out.data_ptr<double>()[i] = rdp_splev1(t.data_ptr<double>(), t.numel(), cc.data_ptr<double>(), k,
                                           x.data_ptr<double>()[i], der);
  return out;
}

// sorted edge points [m,3] -> (ier, mean_k, max_k, spline points [nsamp,3], fp, n)
py::tuple fit_curvature(torch::Tensor pts, double s, int k, int nsamp, double eps) {
  check_cpu_f64(pts, "pts");
  auto out_pts = torch::zeros({nsamp, 3}, torch::kFloat64);
  double out[4] = {0, 0, 0, 0};
  int ier;
  {
    py::gil_scoped_release nogil;
    ier = rdp_fit_curvature(pts.data_ptr<double>(), pts.size(0), s, k, nsamp, eps, out_pts.data_ptr<double>(), out);
  }
  return py::make_tuple(ier, out[0], out[1], out_pts, out[2], (int)out[3]);
}

// geometry: mask u8 [H,W], depth u16-as-int16 [H,W] (GPU) -> packed edge points; returns E via hdr (device)
// m256 (serving form): mask is an OUTPUT (nearest upsample of the model mask) and cov[nblk] gets the
// per-row-block coverage counts; edges None: no packed edge list (hdr untouched)
void geo_edges(torch::Tensor mask, torch::Tensor depth, double fx, double fy, double cx, double cy, double scale,
               torch::Tensor work_i, torch::Tensor work_d, torch::Tensor pts, torch::Tensor npts, torch::Tensor out,
               torch::Tensor kout, int nbins, double top, int min_points, c10::optional<torch::Tensor> edges,
               c10::optional<torch::Tensor> hdr, c10::optional<torch::Tensor> m256, c10::optional<torch::Tensor> cov,
               c10::optional<torch::Tensor> sorted, c10::optional<torch::Tensor> gperm,
               c10::optional<torch::Tensor> mask_host) {
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kUInt8 && mask.dim() == 2 && mask.is_contiguous(), "mask");
  void* mhost = nullptr;
  if (mask_host && mask_host->defined()) {  // pinned / mapped host memory the kernel writes directly
    TORCH_CHECK(!mask_host->is_cuda() && mask_host->scalar_type() == torch::kUInt8 && mask_host->is_contiguous() &&
                    mask_host->numel() == mask.numel(), "mask_host: host u8 tensor of the mask's size");
    TORCH_CHECK(m256 && m256->defined(), "mask_host needs the serving form (m256)");
    mhost = mask_host->data_ptr();
  }
  TORCH_CHECK(depth.is_cuda() && depth.element_size() == 2 && depth.sizes() == mask.sizes() && depth.is_contiguous(),
              "depth u16");
  const int H = mask.size(0), W = mask.size(1);
  const int nblk = rdp_geo_nblocks(H);
  TORCH_CHECK(work_i.numel() >= rdp_geo_work_ints(H, W) && work_i.scalar_type() == torch::kInt32 &&
              work_i.is_contiguous(), "work_i: needs geo_work_ints(H, W) int32");
  TORCH_CHECK(work_d.numel() >= 2 * nblk && work_d.scalar_type() == torch::kFloat64, "work_d");
  TORCH_CHECK(pts.scalar_type() == torch::kFloat64 && pts.numel() >= (long)H * W * 4, "pts cap");
  TORCH_CHECK(out.scalar_type() == torch::kFloat64 && out.dim() == 3 && out.size(0) >= nbins && out.size(2) == 4, "out");
  const bool pack = edges && edges->defined();
  if (pack) {
    TORCH_CHECK(edges->scalar_type() == torch::kFloat64 && edges->dim() == 2 && edges->size(1) == 4, "edges");
    TORCH_CHECK(hdr && hdr->defined() && hdr->scalar_type() == torch::kInt32, "hdr int32");
  }
  const void* mp = nullptr;
  int mh = 0, mw = 0;
  int* covp = nullptr;
  if (m256 && m256->defined()) {
    TORCH_CHECK(m256->is_cuda() && m256->scalar_type() == torch::kUInt8 && m256->dim() == 2 && m256->is_contiguous(),
                "m256 u8 2-D");
    TORCH_CHECK(cov && cov->defined() && cov->scalar_type() == torch::kInt32 && cov->numel() >= nblk,
                "cov: geo_nblocks(H) int32");
    mp = m256->data_ptr();
    mh = m256->size(0);
    mw = m256->size(1);
    covp = cov->data_ptr<int>();
  }
  // sorted (+ gperm): the x-sorted edge points for geo_spline(presorted=True), fused into the select
  double* sp = nullptr;
  int* gp = nullptr;
  int secap = 0;
  if (sorted && sorted->defined()) {
    TORCH_CHECK(sorted->is_cuda() && sorted->scalar_type() == torch::kFloat64 && sorted->dim() == 2 &&
                sorted->size(1) == 3 && sorted->is_contiguous(), "sorted [ecap][3] f64");
    secap = sorted->size(0);
    TORCH_CHECK(gperm && gperm->defined() && gperm->scalar_type() == torch::kInt32 && gperm->numel() >= 2L * secap,
                "gperm: 2*ecap int32");
    sp = sorted->data_ptr<double>();
    gp = gperm->data_ptr<int>();
  }
  const int r = rdp_geo_edges(mask.data_ptr(), depth.data_ptr(), H, W, fx, fy, cx, cy, scale, work_i.data_ptr<int>(),
                              work_d.data_ptr<double>(), work_d.data_ptr<double>() + nblk, pts.data_ptr<double>(), H * W,
                              npts.data_ptr<int>(), out.data_ptr<double>(), out.size(1), kout.data_ptr<int>(), nbins,
                              top, min_points, pack ? edges->data_ptr<double>() : nullptr, pack ? edges->size(0) : 0,
                              pack ? hdr->data_ptr<int>() : nullptr, mp, mh, mw, covp, sp, gp, secap, mhost,
                              unplanned_stream());
  TORCH_CHECK(r >= 0, "geo_edges: nbins must be in [1, 128]");
}

int geo_nblocks(int H) { return rdp_geo_nblocks(H); }
long geo_work_ints(int H, int W) { return rdp_geo_work_ints(H, W); }

// The serving geometry of n <= 4 frames of one camera (BatchEngine): the edge stage (mask upsample +
// coverage, deprojection, bins, per-bin top-k + x-sort) and the spline fit, each ONE launch over the frames
// (csrc/geometry.hip rdp_geo_edges_batch, csrc/geo_spline.hip rdp_geo_spline_batch). Per-frame lists of
// the buffers GeometryEngine.launch_frame / launch_spline pass; the results (and the mask copies) go to
// host memory (res / mask_host).
void geo_frames_batch(std::vector<torch::Tensor> mask, std::vector<torch::Tensor> depth,
                      std::vector<torch::Tensor> m256, std::vector<torch::Tensor> work_i,
                      std::vector<torch::Tensor> work_d, std::vector<torch::Tensor> pts,
                      std::vector<torch::Tensor> npts, std::vector<torch::Tensor> out, std::vector<torch::Tensor> kout,
                      std::vector<torch::Tensor> cov, std::vector<torch::Tensor> sorted,
                      std::vector<torch::Tensor> gperm, std::vector<torch::Tensor> u, std::vector<torch::Tensor> res,
                      std::vector<torch::Tensor> mask_host, double fx, double fy, double cx, double cy, double scale,
                      int nbins, double top, int min_points, double smooth, int k, int nsamp, double eps,
                      int min_edge) {
  const int n = (int)mask.size();
  TORCH_CHECK(n >= 1 && n <= 4, "geo_frames_batch: 1..4 frames");
  for (auto* v : {&depth, &m256, &work_i, &work_d, &pts, &npts, &out, &kout, &cov, &sorted, &gperm, &u, &res})
    TORCH_CHECK((int)v->size() == n, "geo_frames_batch: every list needs one tensor per frame");
  TORCH_CHECK(mask_host.empty() || (int)mask_host.size() == n, "geo_frames_batch: mask_host: none or one per frame");
  const int H = mask[0].size(0), W = mask[0].size(1);
  const int nblk = rdp_geo_nblocks(H);
  const int mh = m256[0].size(0), mw = m256[0].size(1);
  const int cap = H * W, kcap = out[0].size(1), secap = sorted[0].size(0);
  std::vector<const void*> pm(n), pd(n), pm256(n);
  std::vector<int*> pcnt(n), pnpts(n), pkout(n), pcov(n), pgp(n);
  std::vector<double*> pxmin(n), pxmax(n), ppts(n), pout(n), psort(n), pu(n), pres(n);
  std::vector<void*> pmh(n);
  std::vector<const int*> ckout(n), cnpts(n), ccov(n);
  std::vector<const void*> cmask(n);
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(mask[i].is_cuda() && mask[i].scalar_type() == torch::kUInt8 && mask[i].dim() == 2 &&
                    mask[i].is_contiguous() && mask[i].size(0) == H && mask[i].size(1) == W, "mask: u8 HxW, one camera");
    TORCH_CHECK(depth[i].is_cuda() && depth[i].element_size() == 2 && depth[i].sizes() == mask[i].sizes() &&
                    depth[i].is_contiguous(), "depth u16 HxW");
    TORCH_CHECK(m256[i].is_cuda() && m256[i].scalar_type() == torch::kUInt8 && m256[i].dim() == 2 &&
                    m256[i].is_contiguous() && m256[i].size(0) == mh && m256[i].size(1) == mw, "m256 u8 2-D");
    TORCH_CHECK(work_i[i].numel() >= rdp_geo_work_ints(H, W) && work_i[i].scalar_type() == torch::kInt32, "work_i");
    TORCH_CHECK(work_d[i].numel() >= 2 * nblk && work_d[i].scalar_type() == torch::kFloat64, "work_d");
    TORCH_CHECK(pts[i].scalar_type() == torch::kFloat64 && pts[i].numel() >= (long)H * W * 4, "pts cap");
    TORCH_CHECK(out[i].scalar_type() == torch::kFloat64 && out[i].dim() == 3 && out[i].size(0) >= nbins &&
                    out[i].size(1) == kcap && out[i].size(2) == 4 && out[i].is_contiguous(), "out");
    TORCH_CHECK(kout[i].scalar_type() == torch::kInt32 && kout[i].numel() >= nbins, "kout");
    TORCH_CHECK(npts[i].scalar_type() == torch::kInt32, "npts");
    TORCH_CHECK(cov[i].scalar_type() == torch::kInt32 && cov[i].numel() >= nblk, "cov");
    TORCH_CHECK(sorted[i].scalar_type() == torch::kFloat64 && sorted[i].dim() == 2 && sorted[i].size(1) == 3 &&
                    sorted[i].size(0) == secap, "sorted");
    TORCH_CHECK(gperm[i].scalar_type() == torch::kInt32 && gperm[i].numel() >= 2L * secap, "gperm");
    TORCH_CHECK(u[i].scalar_type() == torch::kFloat64 && u[i].numel() >= secap, "u");
    TORCH_CHECK(res[i].scalar_type() == torch::kFloat64 && res[i].numel() >= rdp_geo_spline_res_len(nsamp) &&
                    res[i].is_contiguous(), "res");
    pm[i] = mask[i].data_ptr(); pd[i] = depth[i].data_ptr(); pm256[i] = m256[i].data_ptr();
    pcnt[i] = work_i[i].data_ptr<int>();
    pxmin[i] = work_d[i].data_ptr<double>(); pxmax[i] = pxmin[i] + nblk;
    ppts[i] = pts[i].data_ptr<double>(); pnpts[i] = npts[i].data_ptr<int>(); pout[i] = out[i].data_ptr<double>();
    pkout[i] = kout[i].data_ptr<int>(); pcov[i] = cov[i].data_ptr<int>(); psort[i] = sorted[i].data_ptr<double>();
    pgp[i] = gperm[i].data_ptr<int>(); pu[i] = u[i].data_ptr<double>(); pres[i] = res[i].data_ptr<double>();
    ckout[i] = pkout[i]; cnpts[i] = pnpts[i]; ccov[i] = pcov[i]; cmask[i] = pm[i];
    if (!mask_host.empty()) {
      TORCH_CHECK(!mask_host[i].is_cuda() && mask_host[i].scalar_type() == torch::kUInt8 &&
                      mask_host[i].is_contiguous() && mask_host[i].numel() == mask[i].numel(), "mask_host");
      pmh[i] = mask_host[i].data_ptr();
    }
  }
  const hipStream_t st = unplanned_stream();
  TORCH_CHECK(rdp_geo_edges_batch(n, pm.data(), pd.data(), H, W, fx, fy, cx, cy, scale, pcnt.data(), pxmin.data(),
                                  pxmax.data(), ppts.data(), cap, pnpts.data(), pout.data(), kcap, pkout.data(), nbins,
                                  top, min_points, pm256.data(), mh, mw, pcov.data(), psort.data(), pgp.data(), secap,
                                  nullptr, st) >= 0, "geo_frames_batch: nbins must be in [1, 128]");
  const int r = rdp_geo_spline_batch(n, nbins, kcap, ckout.data(), cnpts.data(), psort.data(), pu.data(), secap,
                                     smooth, k, nsamp, eps, min_points, min_edge, ccov.data(), nblk, pres.data(),
                                     cmask.data(), mask_host.empty() ? nullptr : pmh.data(),
                                     (long)H * W, st);
  TORCH_CHECK(r != -2, "geo_frames_batch: mask copy needs 4-byte aligned buffers and a size multiple of 4");
  TORCH_CHECK(r == 0, "geo_frames_batch: k must be in [1, 5], nsamp in [1, 256]");
}

// on-device spline stage: per-bin sort of the edge points (out/kout from geo_edges) + FITPACK-equivalent
// fit + nsamp-point evaluation and curvature into res (rdp_geo_spline_res_len(nsamp) doubles)
void geo_spline(torch::Tensor out, torch::Tensor kout, torch::Tensor npts, torch::Tensor sorted, torch::Tensor gperm,
                torch::Tensor u, torch::Tensor res, double s, int k, int nsamp, double eps, int min_points,
                int min_edge, c10::optional<torch::Tensor> cov, c10::optional<torch::Tensor> dbg, bool presorted,
                c10::optional<torch::Tensor> mask, c10::optional<torch::Tensor> mask_host) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat64 && out.dim() == 3 && out.size(2) == 4 &&
              out.is_contiguous(), "out [nbins][kcap][4] f64");
  TORCH_CHECK(kout.scalar_type() == torch::kInt32 && kout.numel() >= out.size(0), "kout");
  TORCH_CHECK(npts.scalar_type() == torch::kInt32, "npts int32");
  TORCH_CHECK(sorted.scalar_type() == torch::kFloat64 && sorted.dim() == 2 && sorted.size(1) == 3 &&
              sorted.is_contiguous(), "sorted [ecap][3] f64");
  const int ecap = sorted.size(0);
  TORCH_CHECK(gperm.scalar_type() == torch::kInt32 && gperm.numel() >= 2L * ecap, "gperm: 2*ecap int32");
  TORCH_CHECK(u.scalar_type() == torch::kFloat64 && u.numel() >= ecap, "u: ecap f64");
  TORCH_CHECK(res.scalar_type() == torch::kFloat64 && res.numel() >= rdp_geo_spline_res_len(nsamp), "res");
  const int* covp = nullptr;
  int ncov = 0;
  if (cov && cov->defined()) {
    TORCH_CHECK(cov->scalar_type() == torch::kInt32, "cov int32");
    covp = cov->data_ptr<int>();
    ncov = cov->numel();
  }
  double* dbgp = nullptr;  // optional phase profile (20 doubles, see geo_fit_kernel)
  if (dbg && dbg->defined()) {
    TORCH_CHECK(dbg->is_cuda() && dbg->scalar_type() == torch::kFloat64 && dbg->numel() >= 20, "dbg: >= 20 f64");
    dbgp = dbg->data_ptr<double>();
  }
  // mask + mask_host (serving): the frame mask's host copy, written by blocks beside the fit block
  const void* mp = nullptr;
  void* mh = nullptr;
  long mbytes = 0;
  if (mask_host && mask_host->defined()) {
    TORCH_CHECK(mask && mask->defined() && mask->is_cuda() && mask->scalar_type() == torch::kUInt8 &&
                    mask->is_contiguous(), "geo_spline: mask_host needs the device mask (u8, contiguous)");
    TORCH_CHECK(!mask_host->is_cuda() && mask_host->scalar_type() == torch::kUInt8 && mask_host->is_contiguous() &&
                    mask_host->numel() == mask->numel(), "geo_spline: mask_host: host u8 tensor of the mask's size");
    mp = mask->data_ptr();
    mh = mask_host->data_ptr();
    mbytes = mask->numel();
  }
  const int r = rdp_geo_spline(out.data_ptr<double>(), out.size(0), out.size(1), kout.data_ptr<int>(),
                               npts.data_ptr<int>(), sorted.data_ptr<double>(), gperm.data_ptr<int>(),
                               u.data_ptr<double>(), ecap, s, k, nsamp, eps, min_points, min_edge, covp, ncov,
                               res.data_ptr<double>(), dbgp, presorted ? 1 : 0, mp, mh, mbytes, unplanned_stream());
  TORCH_CHECK(r != -2, "geo_spline: mask copy needs 4-byte aligned buffers and a size multiple of 4");
  TORCH_CHECK(r == 0, "geo_spline: k must be in [1, 5], nsamp in [1, 256]");
}

// INTER_AREA resize of one u8 HxWxC image on the device (tables from data/device_data.py)
void resize_area_u8(torch::Tensor in, torch::Tensor ys, torch::Tensor yn, torch::Tensor yw, torch::Tensor xs,
                    torch::Tensor xn, torch::Tensor xw, int swap_rb, torch::Tensor out) {
  TORCH_CHECK(in.is_cuda() && in.scalar_type() == torch::kUInt8 && in.dim() == 3 && in.is_contiguous(), "in u8 HxWxC");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kUInt8 && out.dim() == 3 && out.is_contiguous() &&
              out.size(2) == in.size(2), "out u8 HxWxC");
  const int H = out.size(0), W = out.size(1), T = rdp_area_maxtap();
  TORCH_CHECK(ys.numel() == H && yn.numel() == H && yw.numel() == (long)H * T && xs.numel() == W &&
              xn.numel() == W && xw.numel() == (long)W * T, "area tables");
  TORCH_CHECK(ys.scalar_type() == torch::kInt32 && yw.scalar_type() == torch::kFloat64, "table dtypes");
  const int r = rdp_resize_area_u8(in.data_ptr(), in.size(0), in.size(1), in.size(2), ys.data_ptr<int>(),
                                   yn.data_ptr<int>(), yw.data_ptr<double>(), xs.data_ptr<int>(), xn.data_ptr<int>(),
                                   xw.data_ptr<double>(), H, W, swap_rb, out.data_ptr(), unplanned_stream());
  TORCH_CHECK(r == 0, "resize_area_u8: C must be 1..4");
}

// Fused batch gather + augmentation (csrc/data_kernels.hip): resident u8 samples idx[0..N) -> the executor's
// x_in (bf16 NHWC8) and target (fp32: one-class mask values; u8: K-class ids, 255 outside the frame).
// Runs outside a launch plan, where UNetExecutor.set_input's copies run.
void batch_augment(torch::Tensor x_res, torch::Tensor y_res, torch::Tensor idx, torch::Tensor params,
                   torch::Tensor x_out, torch::Tensor target) {
  TORCH_CHECK(x_res.is_cuda() && x_res.scalar_type() == torch::kUInt8 && x_res.dim() == 4 && x_res.size(3) == 3 &&
              x_res.is_contiguous(), "batch_augment: x_res u8 [S,H,W,3]");
  const long S = x_res.size(0), H = x_res.size(1), W = x_res.size(2);
  TORCH_CHECK(y_res.is_cuda() && y_res.scalar_type() == torch::kUInt8 && y_res.dim() == 3 && y_res.size(0) == S &&
              y_res.size(1) == H && y_res.size(2) == W && y_res.is_contiguous(), "batch_augment: y_res u8 [S,H,W]");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 && idx.dim() == 1 && idx.is_contiguous(),
              "batch_augment: idx i32 [N]");
  const long N = idx.size(0);
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == torch::kFloat32 && params.dim() == 2 &&
              params.size(0) == N && params.size(1) == 8 && params.is_contiguous(), "batch_augment: params f32 [N,8]");
  TORCH_CHECK(x_out.is_cuda() && x_out.scalar_type() == torch::kBFloat16 && x_out.dim() == 4 && x_out.size(0) == N &&
              x_out.size(1) == H && x_out.size(2) == W && x_out.size(3) == 8 && x_out.is_contiguous() &&
              (uintptr_t)x_out.data_ptr() % 16 == 0, "batch_augment: x_out bf16 [N,H,W,8], 16-byte aligned");
  const bool one_class = target.scalar_type() == torch::kFloat32;
  TORCH_CHECK(target.is_cuda() && (one_class || target.scalar_type() == torch::kUInt8) &&
              target.numel() == N * H * W && target.is_contiguous(), "batch_augment: target f32 | u8 [N*H*W]");
  TORCH_CHECK(S >= 1 && N >= 1 && S <= INT_MAX && N <= INT_MAX, "batch_augment: empty batch or resident set");
  const int r = rdp_batch_augment(x_res.data_ptr(), y_res.data_ptr(), idx.data_ptr<int>(), params.data_ptr<float>(),
                                  (int)S, (int)N, (int)H, (int)W, x_out.data_ptr(),
                                  one_class ? target.data_ptr<float>() : nullptr,
                                  one_class ? nullptr : target.data_ptr(), unplanned_stream());
  TORCH_CHECK(r == 0, "batch_augment: shape outside the kernel");
}

// grayscale 8/16-bit PNG -> u8 / int16 (u16 bits) CPU tensor, decoded without the GIL; None when the
// PNG is not one this reader handles (or is corrupt): the caller falls back to PIL. `parallel`: inflate
// the bands of a banded stream (codecs.cpp) concurrently (2: only that way, else None -- tests).
py::object png_decode(py::bytes data, int parallel) {
  char* buf = nullptr;
  Py_ssize_t n = 0;
  if (PyBytes_AsStringAndSize(data.ptr(), &buf, &n) != 0) throw py::error_already_set();
  int w = 0, h = 0, bd = 0;
  if (rdp_png_info((const uint8_t*)buf, n, &w, &h, &bd) != 0) return py::none();
  auto t = torch::empty({h, w}, torch::TensorOptions().dtype(bd == 16 ? torch::kInt16 : torch::kUInt8));
  int r;
  {
    py::gil_scoped_release nogil;
    r = rdp_png_decode((const uint8_t*)buf, n, (uint8_t*)t.data_ptr(), (long)t.numel() * t.element_size(),
                       parallel);
  }
  if (r != 0) return py::none();
  return py::cast(t);
}

// Baseline JPEG -> (meta int32[32 + 3*64] = geometry + quant tables, quantized coefficient planes int16) on
// the CPU, entropy-decoded without the GIL (restart segments in parallel); None when the stream is not
// one this decoder handles (progressive, arithmetic, 12-bit, ...): the caller falls back to PIL.
// geometry: [0] W, [1] H, [2] ncomp, [3] hmax, [4] vmax, [5] total blocks; per component c at 8 + 8c:
// h, v, blocks per line, block rows, first block, plane byte offset, downsampled width, height.
py::object jpeg_decode(py::bytes data, bool parallel, bool pin) {
  char* buf = nullptr;
  Py_ssize_t n = 0;
  if (PyBytes_AsStringAndSize(data.ptr(), &buf, &n) != 0) throw py::error_already_set();
  int hi[24];
  const long nco = rdp_jpeg_info((const uint8_t*)buf, n, hi);
  if (nco <= 0) return py::none();
  // geometry and quant tables share one int32[32 + 192] tensor (one H2D copy per frame); with `pin`
  // both outputs come from the caching pinned-host allocator so the pipeline's copies are async DMA
  auto opt = torch::TensorOptions().pinned_memory(pin);
  auto meta = torch::zeros({32 + 192}, opt.dtype(torch::kInt32));
  int* g = meta.data_ptr<int>();
  rdp_jpeg_meta(hi, g);
  auto coefs = torch::empty({nco}, opt.dtype(torch::kInt16));
  uint16_t qt16[3 * 64];
  int r;
  {
    py::gil_scoped_release nogil;
    r = rdp_jpeg_decode((const uint8_t*)buf, n, coefs.data_ptr<int16_t>(), nco, qt16, parallel ? 1 : 0);
  }
  if (r != 0) return py::none();
  for (int i = 0; i < 3 * 64; ++i) g[32 + i] = qt16[i];
  return py::make_tuple(meta, coefs);
}

// Dequantisation + ISLOW 8x8 IDCT of every block into the component planes (`planes`, u8 scratch of
// jpeg_plane_bytes(H, W)), then fancy chroma upsampling + YCbCr -> RGB into rgb [H][W][3] u8 (GPU).
// geo / coefs / qt: jpeg_decode's outputs, on the device. Launch sizes come from the pipeline's
// frame size (H, W) so one captured graph serves every JPEG of that size; the kernels read the
// actual geometry from `geo`.
// the pixel stage + preprocess of n <= 4 frames of a serving batch in 2 + 1 launches (BatchEngine): per-frame
// lists; coefs / meta / planes empty for array sources (rgb: HxWx3 u8 colour frames, the preprocess input)
void batch_preprocess(std::vector<torch::Tensor> coefs, std::vector<torch::Tensor> meta,
                      std::vector<torch::Tensor> planes, std::vector<torch::Tensor> rgb, torch::Tensor ystart,
                      torch::Tensor ysize, torch::Tensor yw, torch::Tensor xstart, torch::Tensor xsize,
                      torch::Tensor xw, torch::Tensor out, int rgb_order) {
  const int n = (int)rgb.size();
  TORCH_CHECK(n >= 1 && n <= 4, "batch_preprocess: 1..4 frames");
  const int H = rgb[0].size(0), W = rgb[0].size(1);
  Act o = act(out, "out");
  TORCH_CHECK(o.N >= n && o.C == 8 && o.pitch == 8, "out must be [>= n, OH, OW, 8] contiguous");
  TORCH_CHECK(ystart.numel() == o.H && xstart.numel() == o.W && yw.numel() == (long)o.H * 16 &&
              xw.numel() == (long)o.W * 16, "aa tables");
  const bool jpeg = !coefs.empty();
  TORCH_CHECK(!jpeg || ((int)coefs.size() == n && (int)meta.size() == n && (int)planes.size() == n),
              "batch_preprocess: coefs / meta / planes: one per frame or none");
  std::vector<const void*> pc(n), pr(n);
  std::vector<const int*> pg(n), pq(n);
  std::vector<void*> pp(n), prw(n), po(n);
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(rgb[i].is_cuda() && rgb[i].scalar_type() == torch::kUInt8 && rgb[i].dim() == 3 && rgb[i].size(2) == 3 &&
                    rgb[i].is_contiguous() && rgb[i].size(0) == H && rgb[i].size(1) == W, "rgb u8 HxWx3, one size");
    pr[i] = rgb[i].data_ptr();
    prw[i] = rgb[i].data_ptr();
    po[i] = (char*)o.ptr + (long)i * o.H * o.W * 8 * 2;
    if (jpeg) {
      TORCH_CHECK(coefs[i].is_cuda() && coefs[i].scalar_type() == torch::kInt16 &&
                      coefs[i].numel() >= rdp_jpeg_max_coefs(H, W), "coefs");
      TORCH_CHECK(meta[i].is_cuda() && meta[i].scalar_type() == torch::kInt32 && meta[i].numel() >= 224, "meta");
      TORCH_CHECK(planes[i].is_cuda() && planes[i].numel() >= rdp_jpeg_plane_bytes(H, W), "planes");
      pc[i] = coefs[i].data_ptr();
      pg[i] = meta[i].data_ptr<int>();
      pq[i] = meta[i].data_ptr<int>() + 32;
      pp[i] = planes[i].data_ptr();
    }
  }
  const hipStream_t st = unplanned_stream();
  if (jpeg)
    TORCH_CHECK(rdp_jpeg_gpu_batch(n, pc.data(), pg.data(), pq.data(), pp.data(), H, W,
                                   (int)(coefs[0].numel() / 64), prw.data(), st) == 0, "jpeg batch");
  TORCH_CHECK(rdp_preprocess_batch(n, pr.data(), H, W, ystart.data_ptr<int>(), ysize.data_ptr<int>(),
                                   yw.data_ptr<float>(), xstart.data_ptr<int>(), xsize.data_ptr<int>(),
                                   xw.data_ptr<float>(), o.H, o.W, rgb_order, po.data(), st) == 0, "preprocess batch");
}

void jpeg_to_rgb(torch::Tensor coefs, torch::Tensor geo, torch::Tensor qt, torch::Tensor planes, torch::Tensor rgb) {
  TORCH_CHECK(coefs.is_cuda() && coefs.scalar_type() == torch::kInt16 && coefs.is_contiguous(), "coefs int16");
  TORCH_CHECK(geo.is_cuda() && geo.scalar_type() == torch::kInt32 && geo.numel() >= 32, "geo int32[32]");
  TORCH_CHECK(qt.is_cuda() && qt.scalar_type() == torch::kInt32 && qt.numel() >= 192, "qt int32[192]");
  TORCH_CHECK(rgb.is_cuda() && rgb.scalar_type() == torch::kUInt8 && rgb.dim() == 3 && rgb.size(2) == 3 &&
              rgb.is_contiguous(), "rgb u8 HxWx3");
  const int H = rgb.size(0), W = rgb.size(1);
  TORCH_CHECK(planes.is_cuda() && planes.scalar_type() == torch::kUInt8 && planes.numel() >= rdp_jpeg_plane_bytes(H, W),
              "planes: jpeg_plane_bytes(H, W) u8");
  TORCH_CHECK(coefs.numel() >= rdp_jpeg_max_coefs(H, W), "coefs: jpeg_max_coefs(H, W) int16");
  rdp_jpeg_gpu(coefs.data_ptr(), geo.data_ptr<int>(), qt.data_ptr<int>(), planes.data_ptr(), H, W,
               (int)(coefs.numel() / 64), rgb.data_ptr(), unplanned_stream());
}

// Front end of the GPU entropy decoder (csrc/jpeg.cpp rdp_jpeg_scan): a marker-less baseline JPEG ->
// (meta int32[224] as jpeg_decode's, packed Huffman tables u8, the scan bytes with the 0xFF00 stuffing
// removed and cut at the first marker, nbits), or None where the host decoder has to run (restart markers,
// anything jpeg_decode declines, a scan above `capacity` bytes; 0: sized from the stream). No entropy work.
py::object jpeg_scan(py::bytes data, bool pin, long capacity) {
  char* buf = nullptr;
  Py_ssize_t n = 0;
  if (PyBytes_AsStringAndSize(data.ptr(), &buf, &n) != 0) throw py::error_already_set();
  long cap = capacity;
  if (cap <= 0) cap = rdp_jpeg_scan_bound((const uint8_t*)buf, n);
  if (cap <= 0) return py::none();
  cap = (cap + 3) / 4 * 4;
  auto opt = torch::TensorOptions().pinned_memory(pin);
  auto meta = torch::zeros({32 + 192}, opt.dtype(torch::kInt32));
  auto tables = torch::empty({rdp_jpeg_tables_bytes()}, opt.dtype(torch::kUInt8));
  auto scan = torch::empty({cap}, opt.dtype(torch::kUInt8));
  int nbits = 0, r;
  {
    py::gil_scoped_release nogil;
    r = rdp_jpeg_scan((const uint8_t*)buf, n, meta.data_ptr<int>(), tables.data_ptr<uint8_t>(),
                      scan.data_ptr<uint8_t>(), cap, &nbits);
  }
  if (r != 0) return py::none();
  const long used = std::max(4L, ((long)nbits / 8 + 3) / 4 * 4);
  return py::make_tuple(meta, tables, scan.narrow(0, 0, std::min(used, cap)), nbits);
}

void check_entropy_args(const torch::Tensor& scan, const torch::Tensor& tables, const torch::Tensor& geo,
                        const torch::Tensor& coefs, bool cuda) {
  TORCH_CHECK(scan.is_cuda() == cuda && scan.scalar_type() == torch::kUInt8 && scan.is_contiguous() &&
                  scan.numel() >= 4 && scan.numel() % 4 == 0, "scan: u8, a multiple of 4 bytes");
  TORCH_CHECK(tables.is_cuda() == cuda && tables.scalar_type() == torch::kUInt8 && tables.is_contiguous() &&
                  tables.numel() >= rdp_jpeg_tables_bytes(), "tables: jpeg_scan's u8 block");
  TORCH_CHECK(geo.is_cuda() == cuda && geo.scalar_type() == torch::kInt32 && geo.is_contiguous() && geo.numel() >= 32,
              "geo int32[32]");
  TORCH_CHECK(coefs.is_cuda() == cuda && coefs.scalar_type() == torch::kInt16 && coefs.is_contiguous() &&
                  coefs.numel() >= 64, "coefs int16");
}

// The entropy stage on the GPU (csrc/jpeg_entropy.hip): scan (u8, its numel is the capacity the grids are
// sized from) of which `nbits` bits are the frame's -- an int, or an int32[1] device tensor (a captured
// graph reads the frame's count from it) -- decoded into coefs_out (jpeg_decode's planes). work: int32
// [jpeg_entropy_work_words(scan.numel(), subseq_bits)]; status: int32[1], 0 ok / 1 corrupt after the
// launches (a device tensor, or host memory the device can write). Returns (subsequences, rounds) -- that waits for the stream -- or None while the stream is
// being captured.
py::object jpeg_entropy_gpu(torch::Tensor scan, py::object nbits, torch::Tensor tables, torch::Tensor geo,
                            torch::Tensor coefs_out, torch::Tensor work, torch::Tensor status, int subseq_bits) {
  check_entropy_args(scan, tables, geo, coefs_out, true);
  TORCH_CHECK(work.is_cuda() && work.scalar_type() == torch::kInt32 && work.is_contiguous(), "work int32");
  // status: on the device, or in host memory the device can write (the serving pipeline reads it at
  // collect time without a copy)
  TORCH_CHECK(status.scalar_type() == torch::kInt32 && status.numel() >= 1 && status.is_contiguous(), "status int32[1]");
  int* status_dev = status.data_ptr<int>();
  if (!status.is_cuda()) {
    void* dp = nullptr;
    TORCH_CHECK(hipHostGetDevicePointer(&dp, status.data_ptr(), 0) == hipSuccess && dp,
                "status: a CPU tensor must live in device-mapped host memory");
    status_dev = (int*)dp;
  }
  torch::Tensor nb;
  if (THPVariable_Check(nbits.ptr())) {
    nb = nbits.cast<torch::Tensor>();
    TORCH_CHECK(nb.is_cuda() && nb.get_device() == scan.get_device() && nb.scalar_type() == torch::kInt32 &&
                    nb.numel() >= 1, "nbits: int32[1] on the scan's device");
  } else {
    const long v = nbits.cast<long>();
    TORCH_CHECK(v >= 0 && v <= scan.numel() * 8, "nbits beyond the scan buffer");
    nb = torch::full({1}, v, torch::TensorOptions().dtype(torch::kInt32).device(scan.device()));
  }
  const hipStream_t st = unplanned_stream();
  long stats_word = 0;
  const int r = rdp_jpeg_entropy_gpu(scan.data_ptr(), scan.numel(), nb.data_ptr<int>(), tables.data_ptr(),
                                     geo.data_ptr<int>(), coefs_out.data_ptr(), coefs_out.numel(), work.data_ptr<int>(),
                                     work.numel(), status_dev, subseq_bits, &stats_word, st);
  TORCH_CHECK(r == 0, "jpeg_entropy_gpu: bad arguments (subseq_bits a multiple of 32 >= 64, work of "
                      "jpeg_entropy_work_words, 16-byte aligned tables / coefs) or a failed launch: ", r);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return py::none();
  int stats[2] = {0, 0};
  TORCH_CHECK(hipMemcpyAsync(stats, work.data_ptr<int>() + stats_word, sizeof(stats), hipMemcpyDeviceToHost, st) ==
                  hipSuccess && hipStreamSynchronize(st) == hipSuccess, "jpeg_entropy_gpu: statistics read-back");
  return py::make_tuple(stats[0], stats[1]);
}

// The same stages as plain CPU loops over the shared per-lane code (csrc/jpeg.cpp
// rdp_jpeg_entropy_emulate): CPU tensors, same arguments and results; `work` is not used.
py::object jpeg_entropy_emulate(torch::Tensor scan, py::object nbits, torch::Tensor tables, torch::Tensor geo,
                                torch::Tensor coefs_out, torch::Tensor work, torch::Tensor status, int subseq_bits) {
  check_entropy_args(scan, tables, geo, coefs_out, false);
  TORCH_CHECK(!status.is_cuda() && status.scalar_type() == torch::kInt32 && status.numel() >= 1, "status int32[1]");
  const long v = THPVariable_Check(nbits.ptr()) ? nbits.cast<torch::Tensor>().item<long>() : nbits.cast<long>();
  TORCH_CHECK(v >= 0 && v <= scan.numel() * 8, "nbits beyond the scan buffer");
  int stats[2] = {0, 0}, r;
  {
    py::gil_scoped_release nogil;
    r = rdp_jpeg_entropy_emulate(scan.data_ptr<uint8_t>(), scan.numel(), (int)v, tables.data_ptr<uint8_t>(),
                                 geo.data_ptr<int>(), coefs_out.data_ptr<int16_t>(), coefs_out.numel(), subseq_bits,
                                 status.data_ptr<int>(), stats);
  }
  TORCH_CHECK(r == 0, "jpeg_entropy_emulate: bad arguments (subseq_bits a multiple of 32 >= 64)");
  return py::make_tuple(stats[0], stats[1]);
}

// u8 [H, W] CPU tensor -> 8-bit grayscale PNG bytes (deflate level), encoded without the GIL
// u8 or int16 (u16 bits) [H, W] CPU tensor -> 8 / 16-bit grayscale PNG bytes, encoded without the GIL;
// bands > 1: a banded stream with its rdPs index (codecs.cpp), bands deflated in parallel
py::bytes png_encode(torch::Tensor img, int level, int bands) {
  TORCH_CHECK(!img.is_cuda() && (img.scalar_type() == torch::kUInt8 || img.scalar_type() == torch::kInt16) &&
                  img.dim() == 2 && img.is_contiguous(),
              "u8 / int16 HxW contiguous CPU tensor");
  const int h = img.size(0), w = img.size(1), bpp = (int)img.element_size();
  TORCH_CHECK(h > 0 && w > 0 && level >= 0 && level <= 9 && bands >= 1, "png_encode: bad size / level / bands");
  std::string out((size_t)rdp_png_encode_bound(w, h, bpp, bands), '\0');
  long len;
  {
    py::gil_scoped_release nogil;
    len = rdp_png_encode_gray((const uint8_t*)img.data_ptr(), w, h, bpp, level, bands, (uint8_t*)&out[0],
                              (long)out.size());
  }
  TORCH_CHECK(len > 0, "png encode failed");
  out.resize((size_t)len);
  return py::bytes(out);
}


void preprocess(torch::Tensor bgr, torch::Tensor ystart, torch::Tensor ysize, torch::Tensor yw, torch::Tensor xstart,
                torch::Tensor xsize, torch::Tensor xw, torch::Tensor out, int rgb) {
  TORCH_CHECK(bgr.is_cuda() && bgr.scalar_type() == torch::kUInt8 && bgr.dim() == 3 && bgr.size(2) == 3 &&
              bgr.is_contiguous(), "bgr u8 HxWx3");
  Act o = act(out, "out");
  TORCH_CHECK(o.N == 1 && o.C == 8 && o.pitch == 8, "out must be [1,OH,OW,8] contiguous");
  TORCH_CHECK(ystart.numel() == o.H && xstart.numel() == o.W && yw.numel() == (long)o.H * 16 &&
              xw.numel() == (long)o.W * 16, "aa tables");
  rdp_preprocess(bgr.data_ptr(), bgr.size(0), bgr.size(1), ystart.data_ptr<int>(), ysize.data_ptr<int>(),
                 yw.data_ptr<float>(), xstart.data_ptr<int>(), xsize.data_ptr<int>(), xw.data_ptr<float>(), o.H, o.W,
                 rgb, o.ptr, unplanned_stream());
}

void mask_upsample(torch::Tensor m, torch::Tensor out, torch::Tensor count) {
  TORCH_CHECK(m.is_cuda() && m.scalar_type() == torch::kUInt8 && m.dim() == 2 && m.is_contiguous(), "m");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kUInt8 && out.dim() == 2 && out.is_contiguous(), "out");
  TORCH_CHECK(count.is_cuda() && count.scalar_type() == torch::kInt32, "count int32");
  rdp_mask_upsample(m.data_ptr(), m.size(0), m.size(1), out.data_ptr(), out.size(0), out.size(1),
                    (unsigned*)count.data_ptr(), unplanned_stream());
}

// The serving mask's component filter (csrc/mask_components.hip), in place on n contiguous u8 H x W masks. Every
// refusal is a ValueError and leaves the mask as it was.
void mask_components(torch::Tensor mask, int n, int H, int W, int keep_largest, int min_area,
                     c10::optional<torch::Tensor> stats) {
  TORCH_CHECK_VALUE(n >= 1 && H >= 1 && W >= 1, "mask_components: n, H, W must be >= 1 (got ", n, ", ", H, ", ", W, ")");
  TORCH_CHECK_VALUE((long)H * W <= 65536, "mask_components: H * W = ", (long)H * W, " above 65,536 pixels");
  TORCH_CHECK_VALUE(min_area >= 0, "mask_components: min_area must be >= 0 (got ", min_area, ")");
  TORCH_CHECK_VALUE(mask.is_cuda() && mask.scalar_type() == torch::kUInt8 && mask.is_contiguous() &&
                        mask.numel() >= (long)n * H * W,
                    "mask_components: mask must be a contiguous u8 GPU tensor of n * H * W elements");
  int* sp = nullptr;
  if (stats) {
    TORCH_CHECK_VALUE(stats->is_cuda() && stats->scalar_type() == torch::kInt32 && stats->is_contiguous() &&
                          stats->numel() >= 4l * n,
                      "mask_components: stats must be a contiguous int32 GPU tensor of n * 4 elements");
    sp = stats->data_ptr<int>();
  }
  TORCH_CHECK_VALUE(rdp_mask_components(mask.data_ptr(), n, H, W, keep_largest ? 1 : 0, min_area, sp,
                                        unplanned_stream()) == 0, "mask_components: unsupported arguments");
}

}  // namespace

void register_serve_runtime(py::module_& m);  // serve_runtime.cpp

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_serve_runtime(m);
  m.doc() = "rdp MI355X (gfx950) HIP kernels";
  m.def("stream_wait", &stream_wait, "waiter stream waits for the work issued so far on waitee (recorded in plans)");
  m.def("event_create", &event_create, "runtime-owned cross-stream event (id)");
  m.def("event_record", &event_record, py::arg("id"), py::arg("stream"), "record event id on stream (recorded in plans)");
  m.def("stream_wait_event", &stream_wait_event, py::arg("stream"), py::arg("id"),
        "stream waits for the last record of event id (recorded in plans)");
  m.def("plan_begin", &plan_begin);
  m.def("plan_end", &plan_end);
  m.def("plan_abort", &plan_abort);
  m.def("plan_replay", &plan_replay, py::arg("id"), py::arg("host_call") = py::none());
  m.def("plan_kinds", &plan_kinds);
  m.def("plan_recording", &plan_recording);
  m.def("comm_bind", &comm_bind, "resolve RCCL from the library torch loaded; returns its path");
  m.def("comm_all_reduce", on_device(&comm_all_reduce), py::arg("buf"), py::arg("comm"),
        "in-place SUM all-reduce over an RCCL communicator on the current stream (recorded in plans)");
  m.def("rows_fold", on_device(&rows_fold), py::arg("buf"), py::arg("rows"), py::arg("width"), py::arg("out"));
  m.def("rows_hilo", on_device(&rows_hilo), py::arg("sums"), py::arg("buf"), py::arg("width"));
  m.def("comm_async_error", &comm_async_error, py::arg("comm"), "(code, message) of ncclCommGetAsyncError");
  m.def("comm_abort", &comm_abort, py::arg("comm"), "ncclCommAbort");
  m.def("comm_info", &comm_info, py::arg("comm"), "(ncclCommCount, ncclCommUserRank, ncclCommCuDevice)");
  m.def("comm_emulate", &comm_emulate, py::arg("us"), py::arg("blocks"), py::arg("scratch") = py::none(),
        py::arg("traffic_bytes") = 0, "RDP_DDP_EMULATE: the modelled all-reduce on the current stream (recorded in plans)");
  m.def("plan_mark", &plan_mark, "record a host call point (replay calls host_call(tag) there)");
  m.def("plan_pause", &plan_pause);
  m.def("plan_resume", &plan_resume);
  m.def("plan_size", &plan_size);
  m.def("plan_free", &plan_free);
  m.def("conv_fwd", on_device(&conv_fwd), py::arg("x1"), py::arg("x2"), py::arg("w"), py::arg("taps"), py::arg("packed"),
        py::arg("y1"), py::arg("y2"), py::arg("stats"), py::arg("bm_pref"), py::arg("affine"), py::arg("relu"),
        py::arg("ws") = py::none(), py::arg("pool") = py::none(), py::arg("up") = py::none(),
        py::arg("up_oy") = 0, py::arg("up_ox") = 0, py::arg("wfrag") = py::none(), py::arg("in_coef") = py::none(),
        py::arg("a_out") = py::none());
  m.def("conv_dgrad", on_device(&conv_dgrad), py::arg("dy"), py::arg("w"), py::arg("dx1"), py::arg("dx2") = py::none(),
        py::arg("ws") = py::none(), py::arg("bn_y") = py::none(), py::arg("bn_coef") = py::none(),
        py::arg("bn_partial") = py::none(), py::arg("kernel") = (int)RDP_CONV_AUTO);
  m.def("conv_ws_elems", &rdp_conv_ws_elems);
  m.def("conv_stats_rows", &rdp_conv_stats_rows);
  // the kernels conv_fwd's bm_pref may name (csrc/conv_plan.h RdpConvKernel), as plain ints
  for (int i = 0; i < rdp_conv_kernel_count; ++i)
    m.attr((std::string("CONV_") + rdp_conv_kernel_names[i].name).c_str()) = rdp_conv_kernel_names[i].kernel;
  m.def("conv_plan", &conv_plan, py::arg("n"), py::arg("h"), py::arg("w"), py::arg("c1"), py::arg("c2"), py::arg("cout"),
        py::arg("taps") = 9, py::arg("packed") = 0, py::arg("kernel") = 0, py::arg("stats") = false,
        py::arg("eval") = false, py::arg("split") = 0, py::arg("ws_elems") = 0, py::arg("pool") = false,
        py::arg("up") = false, py::arg("bn") = false, py::arg("wfrag") = false, py::arg("bnin") = false,
        "host only, launches nothing: what conv_fwd / conv_dgrad would run for a dense conv of this shape "
        "(rdp_conv_plan)");
  // the row ring's forms (csrc/conv_plan.h RdpRingForm): conv_plan's ring_form
  m.attr("RING_PLAIN") = (int)RDP_RING_PLAIN; m.attr("RING_POOL") = (int)RDP_RING_POOL;
  m.attr("RING_BNRED") = (int)RDP_RING_BNRED; m.attr("RING_BNIN") = (int)RDP_RING_BNIN;
  m.def("conv_wgrad", on_device(&conv_wgrad), py::arg("x1"), py::arg("x2"), py::arg("dy"), py::arg("taps"),
        py::arg("packed"), py::arg("cin_real"), py::arg("slab"), py::arg("out"), py::arg("accumulate"),
        py::arg("splits"), py::arg("variant"));
  m.def("wgrad_first_bn", on_device(&wgrad_first_bn));
  m.def("wgrad_slab_elems", &rdp_conv_wgrad_slab_elems);
  m.def("wgrad_halo_slab_elems", &rdp_conv_wgrad_halo_slab_elems);
  // the weight-gradient kernels (csrc/conv_plan.h RdpWgradKernel): conv_wgrad's variant takes AUTO, GENERIC, HALO
  for (int i = 0; i < rdp_wgrad_kernel_count; ++i)
    m.attr((std::string("WGRAD_") + rdp_wgrad_kernel_names[i].name).c_str()) = rdp_wgrad_kernel_names[i].kernel;
  m.def("wgrad_plan", &wgrad_plan, py::arg("n"), py::arg("h"), py::arg("w"), py::arg("c1"), py::arg("c2"), py::arg("cout"),
        py::arg("taps") = 9, py::arg("packed") = 0, py::arg("cin_real") = 0, py::arg("kernel") = 0,
        py::arg("splits") = 1, py::arg("slab_elems") = 0, py::arg("upT") = false, py::arg("first_bn") = false,
        "host only, launches nothing: what conv_wgrad / conv_wgrad_upT / wgrad_first_bn would run for a dense layer "
        "of this shape on a slab of slab_elems (rdp_wgrad_plan)");
  m.def("wgrad_auto_splits", &rdp_wgrad_auto_splits, py::arg("n"), py::arg("h"), py::arg("w"), py::arg("cin"),
        py::arg("cout"), py::arg("taps"), py::arg("packed"), py::arg("target_blocks"));
  m.def("bn_finalize", on_device(&bn_finalize));
  m.def("bn_eval_coef", on_device(&bn_eval_coef));
  m.def("bn_relu_apply", on_device(&bn_relu_apply));
  m.def("bn_relu_bwd_reduce", on_device(&bn_relu_bwd_reduce));
  m.def("bn_bwd_finalize", on_device(&bn_bwd_finalize));
  m.def("bn_relu_bwd_apply", on_device(&bn_relu_bwd_apply));
  m.def("maxpool2_fwd", on_device(&maxpool2_fwd));
  m.def("maxpool2_bwd", on_device(&maxpool2_bwd));
  m.def("bn_relu_apply_pool", on_device(&bn_relu_apply_pool));
  m.def("maxpool2_bwd_bn_reduce", on_device(&maxpool2_bwd_bn_reduce));
  m.def("upsample2_fwd", on_device(&upsample2_fwd), py::arg("x"), py::arg("out"), py::arg("oy"), py::arg("ox"),
        py::arg("coef") = py::none());
  m.def("upT_shuffle", on_device(&upT_shuffle));
  m.def("upT_plan", &upT_plan, py::arg("fwd"), py::arg("n"), py::arg("h"), py::arg("w"), py::arg("cin"), py::arg("c"),
        py::arg("h2"), py::arg("w2"), py::arg("oy"), py::arg("ox"));
  m.def("conv_upT_fwd", on_device(&conv_upT_fwd));
  m.def("conv_upT_dgrad", on_device(&conv_upT_dgrad));
  m.def("conv_wgrad_upT", on_device(&conv_wgrad_upT));
  m.def("upT_unshuffle", on_device(&upT_unshuffle));
  m.def("colsum_bf16", on_device(&colsum_bf16));
  m.def("upsample2_bwd", on_device(&upsample2_bwd), py::arg("dout"), py::arg("dx"), py::arg("oy"), py::arg("ox"),
        py::arg("y") = py::none(), py::arg("coef") = py::none(), py::arg("partial") = py::none());
  m.def("head_partial_blocks", &head_partial_blocks);
  m.def("head_fwd", on_device(&head_fwd), py::arg("a"), py::arg("w"), py::arg("b"), py::arg("target"), py::arg("logits"),
        py::arg("partial"), py::arg("sums"), py::arg("loss"), py::arg("dice_w"), py::arg("dice_eps"),
        py::arg("coef") = py::none(), py::arg("gpart") = py::none(), py::arg("bnpart") = py::none(),
        py::arg("gscale") = 1.0);
  m.def("head_grad_finalize", on_device(&head_grad_finalize));
  m.def("head_bwd", on_device(&head_bwd), py::arg("a"), py::arg("w"), py::arg("logits"), py::arg("target"), py::arg("sums"),
        py::arg("da"), py::arg("partial"), py::arg("gw"), py::arg("gb"), py::arg("dice_w"), py::arg("dice_eps"),
        py::arg("gscale"), py::arg("coef") = py::none(), py::arg("bnpart") = py::none());
  m.def("head_bn_bwd_apply", on_device(&head_bn_bwd_apply));
  m.def("head_mask", on_device(&head_mask));
  m.def("headk_partial_blocks", &headk_partial_blocks);
  m.def("headk_fwd", on_device(&headk_fwd), py::arg("a"), py::arg("w"), py::arg("b"), py::arg("labels"),
        py::arg("logits"), py::arg("partial"), py::arg("sums"), py::arg("loss"), py::arg("class_weights") = py::none(),
        py::arg("dice_w") = 0.0, py::arg("dice_eps") = 1.0);
  m.def("headk_bwd", on_device(&headk_bwd), py::arg("a"), py::arg("w"), py::arg("logits"), py::arg("labels"),
        py::arg("sums"), py::arg("da"), py::arg("partial"), py::arg("gw"), py::arg("gb"), py::arg("gscale") = 1.0,
        py::arg("class_weights") = py::none(), py::arg("dice_w") = 0.0, py::arg("dice_eps") = 1.0);
  m.def("headk_mask", on_device(&headk_mask), py::arg("a"), py::arg("w"), py::arg("b"), py::arg("cls"),
        py::arg("mask"));
  m.def("seg_confusion_blocks", &seg_confusion_blocks);
  m.def("seg_confusion_block_pixels", &seg_confusion_block_pixels);
  m.def("seg_confusion", on_device(&seg_confusion), py::arg("logits"), py::arg("target"), py::arg("K"),
        py::arg("counts"), py::arg("thr") = 0.0, py::arg("max_blocks") = 0);
  m.def("conv_head_mask", on_device(&conv_head_mask));
  m.def("conv_headk_mask", on_device(&conv_headk_mask), py::arg("x"), py::arg("w"), py::arg("coef"), py::arg("head_w"),
        py::arg("head_b"), py::arg("cls"), py::arg("mask"));
  m.def("conv_rowband_chain", on_device(&conv_rowband_chain));
  m.def("conv_rowband", on_device(&conv_rowband));
  // host-only: the eval conv's row-band mode for a shape (0 = implicit GEMM), the same decision conv_fwd takes
  m.def("rowband_frag_mode", &rdp_rowband_frag_mode, py::arg("n"), py::arg("h"), py::arg("w"), py::arg("c1"),
        py::arg("c2"), py::arg("cout"));
  m.def("adam", on_device(&adam), py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("lr"),
        py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("gscale"), py::arg("step"),
        py::arg("inc") = true, py::arg("max_blocks") = 0);
  m.def("grad_sqnorm_blocks", &grad_sqnorm_blocks, py::arg("n"));
  m.def("grad_sqnorm", on_device(&grad_sqnorm), py::arg("g"), py::arg("partial"), py::arg("max_blocks") = 0);
  m.def("optim_ctl", on_device(&optim_ctl), py::arg("partial"), py::arg("nblocks"), py::arg("gscale"), py::arg("clip"),
        py::arg("sched"), py::arg("warmup"), py::arg("total"), py::arg("min_ratio"), py::arg("step"), py::arg("ctl"));
  m.def("adam_ctl", on_device(&adam_ctl), py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("gscale"), py::arg("step"),
        py::arg("ctl"), py::arg("inc") = true, py::arg("max_blocks") = 0);
  m.def("cast_bf16", on_device(&cast_bf16));
  m.def("h2d_copy", &h2d_copy, py::arg("src"), py::arg("dst"));
  m.def("wprep", on_device(&wprep), py::arg("master"), py::arg("out"), py::arg("segs"), py::arg("nseg"),
        py::arg("step") = py::none(), py::arg("blocks") = 0);
  m.def("wseg_size", &rdp_wseg_size);
  m.def("parcur", &parcur);
  m.def("batch_preprocess", on_device(&batch_preprocess));
  m.def("geo_frames_batch", on_device(&geo_frames_batch));
  m.def("geo_edges", on_device(&geo_edges), py::arg("mask"), py::arg("depth"), py::arg("fx"), py::arg("fy"), py::arg("cx"),
        py::arg("cy"), py::arg("scale"), py::arg("work_i"), py::arg("work_d"), py::arg("pts"), py::arg("npts"),
        py::arg("out"), py::arg("kout"), py::arg("nbins"), py::arg("top"), py::arg("min_points"),
        py::arg("edges") = py::none(), py::arg("hdr") = py::none(), py::arg("m256") = py::none(),
        py::arg("cov") = py::none(), py::arg("sorted") = py::none(), py::arg("gperm") = py::none(),
        py::arg("mask_host") = py::none());
  m.def("geo_nblocks", &geo_nblocks);
  m.def("geo_spline", on_device(&geo_spline), py::arg("out"), py::arg("kout"), py::arg("npts"), py::arg("sorted"),
        py::arg("gperm"), py::arg("u"), py::arg("res"), py::arg("s"), py::arg("k"), py::arg("nsamp"), py::arg("eps"),
        py::arg("min_points"), py::arg("min_edge"), py::arg("cov") = py::none(), py::arg("dbg") = py::none(),
        py::arg("presorted") = false, py::arg("mask") = py::none(), py::arg("mask_host") = py::none());
  m.def("png_decode", &png_decode, py::arg("data"), py::arg("parallel") = 1,
        "parallel: 0 serial inflate, 1 banded (rdPs index) with serial fallback, 2 banded only (tests)");
  m.def("jpeg_decode", &jpeg_decode, py::arg("data"), py::arg("parallel") = true, py::arg("pin") = false);
  m.def("jpeg_to_rgb", on_device(&jpeg_to_rgb));
  m.def("jpeg_plane_bytes", &rdp_jpeg_plane_bytes);
  m.def("jpeg_scan", &jpeg_scan, py::arg("data"), py::arg("pin") = false, py::arg("capacity") = 0);
  m.def("jpeg_entropy_gpu", on_device(&jpeg_entropy_gpu), py::arg("scan"), py::arg("nbits"), py::arg("tables"),
        py::arg("geo"), py::arg("coefs_out"), py::arg("work"), py::arg("status"), py::arg("subseq_bits") = 0);
  m.def("jpeg_entropy_emulate", &jpeg_entropy_emulate, py::arg("scan"), py::arg("nbits"), py::arg("tables"),
        py::arg("geo"), py::arg("coefs_out"), py::arg("work"), py::arg("status"), py::arg("subseq_bits") = 0);
  m.def("jpeg_entropy_work_words", &rdp_jpeg_entropy_work_words);
  m.def("jpeg_tables_bytes", &rdp_jpeg_tables_bytes);
  m.def("jpeg_max_coefs", &rdp_jpeg_max_coefs);
  m.def("png_encode", &png_encode, py::arg("img"), py::arg("level") = 1, py::arg("bands") = 1);
  m.def("resize_area_u8", on_device(&resize_area_u8));
  m.def("area_maxtap", &rdp_area_maxtap);
  m.def("batch_augment", on_device(&batch_augment));
  m.def("geo_spline_res_len", &rdp_geo_spline_res_len);
  m.def("geo_work_ints", &geo_work_ints);
  m.def("preprocess", on_device(&preprocess), py::arg("bgr"), py::arg("ystart"), py::arg("ysize"), py::arg("yw"),
        py::arg("xstart"), py::arg("xsize"), py::arg("xw"), py::arg("out"), py::arg("rgb") = 0);
  m.def("mask_upsample", on_device(&mask_upsample));
  m.def("mask_components", on_device(&mask_components), py::arg("mask"), py::arg("n"), py::arg("H"), py::arg("W"),
        py::arg("keep_largest"), py::arg("min_area"), py::arg("stats") = py::none());
  m.def("splev", &splev);
  m.def("fit_curvature", &fit_curvature);
}
