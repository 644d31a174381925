// runtime.hip — the library's own state and its thin wrappers of the HIP runtime: the thread-local
// error string behind gnn::fail / gnn_last_error, gnn_version, and the calls Python has no other way
// to make (host registration, CU-masked streams, an async host-to-device copy, IPC export / open /
// close). No kernels.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gnn_spmm.h"
#include "common.h"

#ifndef GNN_BUILD_ID
#define GNN_BUILD_ID "dev"
#endif

namespace {
thread_local std::string g_err;
}  // namespace

int gnn::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" {

const char* gnn_last_error(void) { return g_err.c_str(); }

const char* gnn_version(void) { return "gnn_spmm gfx950 " GNN_BUILD_ID; }

int gnn_host_register(void* host, size_t bytes) {
  GNN_REQUIRE(host && bytes > 0, "gnn_host_register: NULL or empty range");
  GNN_HIP(hipHostRegister(host, bytes, hipHostRegisterMapped), "hipHostRegister");
  return 0;
}

int gnn_host_unregister(void* host) {
  GNN_REQUIRE(host, "gnn_host_unregister: NULL");
  GNN_HIP(hipHostUnregister(host), "hipHostUnregister");
  return 0;
}

int gnn_stream_create_cu_masked(int32_t device, int32_t cus, int32_t priority, void** stream_out) {
  GNN_REQUIRE(stream_out, "gnn_stream_create_cu_masked: NULL stream_out");
  *stream_out = nullptr;
  GNN_HIP(hipSetDevice(device), "hipSetDevice");
  int ncu = 0;
  GNN_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device), "hipDeviceGetAttribute");
  GNN_REQUIRE(cus > 0 && cus <= ncu, "gnn_stream_create_cu_masked: cus must be in [1, %d]", ncu);
  std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
  const int stride = ncu / cus;  // spread over the device's CU numbering (every XCD gets its share)
  for (int i = 0, k = 0; i < ncu && k < cus; i += stride, ++k) mask[(size_t)i / 32] |= 1u << (i % 32);
  hipStream_t st = nullptr;
  GNN_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()), "hipExtStreamCreateWithCUMask");
  (void)priority;
  *stream_out = (void*)st;
  return 0;
}

int gnn_stream_destroy(void* stream) {
  if (stream) GNN_HIP(hipStreamDestroy((hipStream_t)stream), "hipStreamDestroy");
  return 0;
}

int gnn_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream) {
  if (bytes == 0) return 0;
  GNN_REQUIRE(dst && src, "gnn_memcpy_h2d_async: NULL pointer");
  GNN_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync");
  return 0;
}

int gnn_ipc_export(const void* ptr, void* handle_out, int64_t* offset_out) {
  GNN_REQUIRE(ptr && handle_out && offset_out, "gnn_ipc_export: NULL argument");
  static_assert(sizeof(hipIpcMemHandle_t) == GNN_IPC_HANDLE_BYTES, "IPC handle size");
  void* base = nullptr;
  size_t size = 0;
  GNN_HIP(hipMemGetAddressRange(&base, &size, const_cast<void*>(ptr)), "hipMemGetAddressRange");
  hipIpcMemHandle_t h;
  GNN_HIP(hipIpcGetMemHandle(&h, base), "hipIpcGetMemHandle");
  std::memcpy(handle_out, &h, sizeof(h));
  *offset_out = (int64_t)((const char*)ptr - (const char*)base);
  return 0;
}

int gnn_ipc_open(const void* handle, int64_t offset, int peer_device, void** ptr_out) {
  GNN_REQUIRE(handle && ptr_out && offset >= 0, "gnn_ipc_open: bad argument");
  int cur = 0;
  GNN_HIP(hipGetDevice(&cur), "hipGetDevice");
  if (peer_device >= 0 && peer_device != cur) {
    int can = 0;
    GNN_HIP(hipDeviceCanAccessPeer(&can, cur, peer_device), "hipDeviceCanAccessPeer");
    GNN_REQUIRE(can, "gnn_ipc_open: this GPU cannot access the peer GPU's memory");
    const hipError_t e = hipDeviceEnablePeerAccess(peer_device, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
    else GNN_HIP(e, "hipDeviceEnablePeerAccess");
  }
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, sizeof(h));
  void* base = nullptr;
  GNN_HIP(hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
  *ptr_out = (char*)base + offset;
  return 0;
}

int gnn_ipc_close(void* ptr, int64_t offset) {
  GNN_REQUIRE(ptr && offset >= 0, "gnn_ipc_close: bad argument");
  GNN_HIP(hipIpcCloseMemHandle((char*)ptr - offset), "hipIpcCloseMemHandle");
  return 0;
}

}  // extern "C"
