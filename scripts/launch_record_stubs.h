// The part of the HIP runtime that a HOST-ONLY build of a csrc/*.hip file needs, as recording stubs shared by the launch recorders
// (scripts/fwd_launch_record.hip, scripts/gemm_launch_record.hip): every enqueue goes as text to the file named by SHIM_LOG, nothing runs and
// no GPU is needed.  The including stand-in defines dump_launch_args(): the kernel arguments of one launch, by registered kernel name.
#pragma once
#include "gemm_shared.h"
#include <cstdio>
#include <cstdarg>
#include <map>
#include <string>
static FILE* out() { static FILE* f = fopen(getenv("SHIM_LOG"), "w"); return f; }
static std::map<const void*, std::string>& names() { static std::map<const void*, std::string> m; return m; }
static void dump_launch_args(const std::string& kernel, void** args);
static char g_err[512];
void evc_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
extern "C" {
char __hip_fatbin[64];
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, int, void*, void*, void*, void*, int*) { names()[host] = name; }
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
static dim3 g_grid, g_block; static size_t g_sh; static hipStream_t g_st;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t st) { g_grid = g; g_block = b; g_sh = sh; g_st = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* st) { *g = g_grid; *b = g_block; *sh = g_sh; *st = g_st; return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** a, size_t sh, hipStream_t st) {
  const std::string& n = names()[f];
  fprintf(out(), "launch %s grid=%u block=%u lds=%zu stream=%p\n", n.c_str(), g.x, b.x, sh, (void*)st);
  dump_launch_args(n, a);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t st) { fprintf(out(), "memset %p %d %zu\n", p, v, n); return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "?"; }
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute, int v) { fprintf(out(), "attr %s %d\n", names()[f].c_str(), v); return hipSuccess; }
void shim_note(const char* s) { fprintf(out(), "%s\n", s); fflush(out()); }
const char* shim_err() { return g_err; }
void shim_clear_err() { g_err[0] = 0; }
}
