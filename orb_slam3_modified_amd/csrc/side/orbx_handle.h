// The host-side core of a side library's handle (liborbx_stereo.so, liborbx_bow.so, liborbx_match.so, liborbx_initmatch.so: DESIGN.md
// sections 10 and 11).  Host code only; it sits below csrc/, outside kernels_hash().  A handle derives from orbx::side::Handle and adds what
// is its own.  Each family's host layer is beside this file: the four pair matchers' in orbx_pair_host.h (their device helpers in
// orbx_pair_device.h), the four chained projection matchers' in orbx_window_host.h, the three projection fronts' in orbx_front_host.h.
//
// The rule it keeps: the calls on one handle share its scratch, so each waits for the one before it (wait_previous / record_call around
// ev_done), and a block of the handle is replaced only once the handle is idle (grow behind quiesce).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../../include/orbx.h"

namespace orbx {
namespace side {

struct Block { uint8_t* p = nullptr; size_t bytes = 0; };   // a grow-only device allocation

struct Handle {
  int device = 0;
  hipStream_t st = nullptr;        // the host forms' copies and kernels; a device form without a stream argument
  hipEvent_t ev_done = nullptr;
  bool pending = false;            // ev_done recorded: the previous call's work may still use the scratch
  Block scratch;                   // the kernels' intermediate buffers
  Block io;                        // the host forms' device copies of arguments and results
  std::vector<uint8_t> h_io;       // the host forms' results before they are handed out
  std::string err;
};

struct Layout {                    // offsets in one block, 256-byte aligned
  size_t size = 0;
  size_t add(size_t bytes) { const size_t o = size; size = (size + bytes + 255) & ~(size_t)255; return o; }
};

// an integer from the environment, clamped to [lo, hi]; `fallback` when the variable is not set
inline int env_int(const char* name, int lo, int hi, int fallback) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : fallback;
}

inline thread_local std::string t_create_err;   // why the last create of this thread failed: there is no handle to hold it

inline int fail(Handle* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}
inline int create_fail(int code, const char* who, const char* msg) {
  t_create_err = std::string(who) + ": " + msg;
  return code;
}
inline const char* last_error(const Handle* h) { return h ? h->err.c_str() : t_create_err.c_str(); }

// returns ORBX_E_DEVICE from the calling function, with the runtime's sticky error cleared
#define ORBX_SIDE_HIP(h, expr)                                                                                 \
  do {                                                                                                         \
    const hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) {                                                                                    \
      (void)hipGetLastError();                                                                                 \
      return orbx::side::fail((h), ORBX_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    }                                                                                                          \
  } while (0)

// the handle's previous work is over and its stream idle: a block of the handle may be replaced
inline int quiesce(Handle* h) {
  if (h->pending) ORBX_SIDE_HIP(h, hipEventSynchronize(h->ev_done));
  h->pending = false;
  ORBX_SIDE_HIP(h, hipStreamSynchronize(h->st));
  return ORBX_OK;
}

// calls on one handle share its scratch: one after the other
inline int wait_previous(Handle* h, hipStream_t st) {
  if (h->pending) ORBX_SIDE_HIP(h, hipStreamWaitEvent(st, h->ev_done, 0));
  return ORBX_OK;
}
// after a call's last launch on `st`: the launches went through, and the next call waits for them
inline int record_call(Handle* h, hipStream_t st) {
  ORBX_SIDE_HIP(h, hipGetLastError());
  ORBX_SIDE_HIP(h, hipEventRecord(h->ev_done, st));
  h->pending = true;
  return ORBX_OK;
}
// the tail of a host form: everything queued on the handle's stream is done, the results are in the caller's memory
inline int finish_host(Handle* h) {
  ORBX_SIDE_HIP(h, hipStreamSynchronize(h->st));
  h->pending = false;
  return ORBX_OK;
}

inline int grow(Handle* h, Block* b, size_t bytes) {
  if (bytes <= b->bytes) return ORBX_OK;
  const int rc = quiesce(h);             // the previous call may still use the old block
  if (rc != ORBX_OK) return rc;
  if (b->p) (void)hipFree(b->p);
  b->p = nullptr; b->bytes = 0;
  ORBX_SIDE_HIP(h, hipMalloc((void**)&b->p, bytes));
  b->bytes = bytes;
  return ORBX_OK;
}

// the device a pointer lives on, -1 when the runtime does not know it (then nothing is concluded from it)
inline int pointer_device(const void* p) {
  hipPointerAttribute_t at;
  if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return at.type == hipMemoryTypeDevice ? at.device : -1;
}

// every buffer the runtime knows lives on the handle's device; `owner` names in the message what the handle's device is that of
inline int same_device(Handle* h, const char* who, std::initializer_list<const void*> buffers, const char* owner) {
  for (const void* p : buffers) {
    const int pd = pointer_device(p);
    if (pd >= 0 && pd != h->device)
      return fail(h, ORBX_E_INVALID, std::string(who) + "a buffer lives on device " + std::to_string(pd) + ", " + owner + " on device " + std::to_string(h->device));
  }
  return ORBX_OK;
}

// a kernel may be launched with up to `bytes` of dynamic LDS; what failed, or nullptr
inline const char* allow_lds(const void* kernel, int bytes) {
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) return nullptr;
  (void)hipGetLastError();
  return "the kernel's LDS size was refused";
}

// A host form's arguments and results in the handle's io block.  The form declares its inputs, then its results (which lie together at the
// end of the block), each call returning the offset in the block; upload() queues the inputs' copies in the order of their declaration, the
// form calls its device form on h->io.p + offset, and download() reads the results back in one copy and hands them out.
struct Stager {
  struct Item { size_t off, bytes; const void* src; void* dst; };
  Layout lay;
  size_t o_out = 0;                // where the results begin
  std::vector<Item> ins, outs;
  size_t in(const void* host, size_t bytes) {
    const size_t o = lay.add(bytes);
    ins.push_back({o, bytes, host, nullptr});
    return o;
  }
  // `host` null: the result has its place but is not handed out.  `both`: what `host` holds is uploaded first (an argument that is updated)
  size_t out(void* host, size_t bytes, bool both = false) {
    if (outs.empty()) o_out = lay.size;
    const size_t o = lay.add(bytes);
    if (both && host) ins.push_back({o, bytes, host, nullptr});
    outs.push_back({o, bytes, nullptr, host});
    return o;
  }
};

inline int upload(Handle* h, const Stager& s) {
  ORBX_SIDE_HIP(h, hipSetDevice(h->device));
  int rc = grow(h, &h->io, s.lay.size);
  if (rc != ORBX_OK) return rc;
  if ((rc = wait_previous(h, h->st)) != ORBX_OK) return rc;
  for (const Stager::Item& i : s.ins) ORBX_SIDE_HIP(h, hipMemcpyAsync(h->io.p + i.off, i.src, i.bytes, hipMemcpyHostToDevice, h->st));
  return ORBX_OK;
}

inline int download(Handle* h, const Stager& s) {
  const size_t bytes = s.lay.size - s.o_out;
  if (h->h_io.size() < bytes) h->h_io.resize(bytes);
  ORBX_SIDE_HIP(h, hipMemcpyAsync(h->h_io.data(), h->io.p + s.o_out, bytes, hipMemcpyDeviceToHost, h->st));
  const int rc = finish_host(h);
  if (rc != ORBX_OK) return rc;
  for (const Stager::Item& o : s.outs)
    if (o.dst) std::memcpy(o.dst, h->h_io.data() + o.off - s.o_out, o.bytes);
  return ORBX_OK;
}

// the handle's stream and event on `device`; what failed, or nullptr.  close_handle() takes a half-opened handle too
inline const char* open_handle(Handle* h, int device) {
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return "hipSetDevice failed"; }
  if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    return "stream / event creation failed";
  }
  return nullptr;
}
inline void close_handle(Handle* h) {
  (void)hipSetDevice(h->device);
  if (h->pending && h->ev_done) (void)hipEventSynchronize(h->ev_done);
  if (h->st) (void)hipStreamSynchronize(h->st);
  if (h->scratch.p) (void)hipFree(h->scratch.p);
  if (h->io.p) (void)hipFree(h->io.p);
  if (h->ev_done) (void)hipEventDestroy(h->ev_done);
  if (h->st) (void)hipStreamDestroy(h->st);
}

// The create of a library whose handle is made from a device number alone: `who` is the entry point's name in the messages, init(handle)
// reads the library's environment and raises its kernels' LDS limits (allow_lds) on the opened device: what failed, or nullptr.
template <class H, class Init>
int create_handle(H** out, int device, const char* who, void (*destroy)(H*), Init init) {
  if (out) *out = nullptr;
  if (!out) return create_fail(ORBX_E_INVALID, who, "null argument");
  if (device < 0) return create_fail(ORBX_E_INVALID, who, "device must be >= 0");
  H* h = new H();
  const char* e = open_handle(h, device);
  if (!e) e = init(h);
  if (e) { destroy(h); return create_fail(ORBX_E_DEVICE, who, e); }
  *out = h;
  return ORBX_OK;
}
template <class H>
void destroy_handle(H* h) {
  if (!h) return;
  close_handle(h);
  delete h;
}

// Where a chunked window kernel keeps its arrays.  It needs `fixed_lds` bytes of arrays and room for one query's longest list (`longest`
// candidates of 4 bytes); when that fits the handle's LDS limit, what is left of the limit is candidate room.  Otherwise every workgroup
// gets a slice of the handle's scratch (grown here): `fixed_global` bytes and a room of at least global_room candidates.
struct PathLimits { int lds_blocks, global_blocks, global_room; };
struct Paths { bool in_lds; size_t lds_bytes; int room, blocks; size_t scratch_stride; };
inline int plan_paths(Handle* h, int lds_limit, size_t fixed_lds, size_t fixed_global, int longest, int items, PathLimits lim, Paths* p) {
  const size_t limit = (size_t)lds_limit & ~(size_t)15;
  p->in_lds = fixed_lds + 4 * (size_t)longest <= limit;
  if (p->in_lds) {
    *p = {true, limit, (int)((limit - fixed_lds) / 4), std::min(items, lim.lds_blocks), 0};
    return ORBX_OK;
  }
  const int room = std::max(longest, lim.global_room), blocks = std::min(items, lim.global_blocks);
  *p = {false, 0, room, blocks, (fixed_global + 4 * (size_t)room + 255) & ~(size_t)255};
  return grow(h, &h->scratch, p->scratch_stride * blocks);
}

}  // namespace side
}  // namespace orbx
