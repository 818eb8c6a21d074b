// What the host-side checks of the evaluation entries share (tools/*_hostcheck.cpp: stand-alone programs built with
// AddressSanitizer and UBSan on the library's HOST code, run on a machine without a GPU, never loaded into Python).
// A program defines its `struct Args`, `Args pointing_at(void*)`, `oetr_status call(const Args&)` and the name of its
// entry point, `const char ENTRY[]`; its main() is
//
//   hostcheck::begin();
//   const Args good = pointing_at(hostcheck::keep);  Args a;
//   REJECT("maps = NULL", a.maps = nullptr, OETR_ERR_BAD_ARG);  ...      1. every rejected-argument path
//   if (char* none = hostcheck::no_device_page()) {                      2. acceptable arguments, PROT_NONE pointers
//     a = pointing_at(none + 256);  ...  hostcheck::expect_no_device("label", a);
//   }
//   return hostcheck::finish();
#pragma once
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/oetr_hip.h"

namespace hostcheck {

inline int failures = 0;
// 64 host bytes that stand in for the device in the rejected calls: no call may touch them
alignas(16) inline unsigned char keep[64];
constexpr size_t PAGE = 1 << 16;
inline void* page = nullptr;

inline void begin() { std::memset(keep, 0xA5, sizeof keep); }

// A rejected call: returns `want`, sets an oetr_last_error that opens with the entry's name, leaves `keep` alone.
template <class Args>
void expect(const char* entry, const char* what, const Args& a, oetr_status want) {
  const oetr_status got = call(a);
  const char* msg = oetr_last_error();
  bool ok = got == want && msg && std::strncmp(msg, entry, std::strlen(entry)) == 0;
  for (unsigned char c : keep) ok = ok && c == 0xA5;
  std::printf("%-32s status %d (want %d) %s\n", what, (int)got, (int)want, ok ? "ok" : "FAILED");
  if (!ok) {
    std::printf("    last error: %s\n", msg ? msg : "(null)");
    ++failures;
  }
}

// `a` = the program's `good` arguments with one edit, refused with `status`
#define REJECT(name, edit, status) \
  a = good;                        \
  edit;                            \
  hostcheck::expect(ENTRY, name, a, status)

// A PROT_NONE page for the calls whose "device" pointers nobody may dereference - or nullptr where a GPU is visible:
// those calls would enqueue kernels on host addresses, so they are SKIPPED and the program says so.
inline char* no_device_page() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
    std::printf("a GPU is visible: the PROT_NONE calls are SKIPPED (they would enqueue on host addresses); run this "
                "program on a machine without one\n");
    return nullptr;
  }
  (void)hipGetLastError();
  page = mmap(nullptr, PAGE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (page == MAP_FAILED) {
    std::perror("mmap");
    std::exit(1);
  }
  return static_cast<char*>(page);
}

// An acceptable call on PROT_NONE pointers: the host code dereferences none of them, so it comes back with a status
// (OETR_ERR_HIP: there is no device to enqueue on), not with a signal.
template <class Args>
void expect_no_device(const char* label, const Args& a) {
  const oetr_status got = call(a);
  const bool ok = got == OETR_ERR_HIP;
  std::printf("PROT_NONE, %-28s status %d (want %d: no device) %s\n    last error: %s\n", label, (int)got,
              (int)OETR_ERR_HIP, ok ? "ok" : "FAILED", oetr_last_error());
  failures += !ok;
}

// the closing line and main()'s return value
inline int finish() {
  if (page) munmap(page, PAGE);
  std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}

}  // namespace hostcheck
