// hostlib/err.h -- the calling thread's last error text (vgl_last_error), the check of a HIP call and the environment hooks.
// Part of the one translation unit vgl_host.cpp.
#pragma once

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}
// a call of this library that has already set the error text
#define VGLCHK(call) do { const int rc_ = (call); if (rc_ != VGL_OK) return rc_; } while (0)

#ifndef VGL_MEM_TEST                   // (the CPU programs of mem.h and batch.h take fail() and VGLCHK alone: nothing of HIP)
static int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? VGL_E_NOMEM : VGL_E_NODEVICE; }
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(hip_code(e_), "%s: %s", #call, hipGetErrorString(e_)); } while (0)

// Environment overrides (tuning switches and test hooks) exist only in the -DVGL_TEST_HOOKS build of the library
// (lib/libvcfgl_hip_hooks.so, what the test-suite's hook cases and tools/ load): the shipped library reads no environment variable.
#ifdef VGL_TEST_HOOKS
static const char* hook_env(const char* name) { return getenv(name); }
#else
static const char* hook_env(const char*) { return nullptr; }
#endif

extern "C" const char* vgl_last_error(void) { return g_err; }
extern "C" int vgl_abi_version(void) { return VGL_ABI_VERSION; }
extern "C" int vgl_pack_set_error(int code, const char* msg);      // (vgl_pack.hip reports through vgl_last_error() too; not exported)
extern "C" int vgl_pack_set_error(int code, const char* msg) { return fail(code, "%s", msg); }
#endif
