// Enumerates, without a GPU, which kernels libhdmoe_hip.so's conv entry points launch over a grid of layer shapes.
//
//   hipcc -O1 -std=c++17 -rdynamic tools/launch_enum.cpp -o launch_enum -ldl && ./launch_enum path/to/libhdmoe_hip.so > launches.txt
//
// The program defines hipLaunchKernel (and the few HIP calls the host dispatch makes) itself, so the library's launches land here: one
// output line per launch with the call number, the kernel's demangled name, grid, block, dynamic LDS and a hash of the kernarg bytes
// (padding and fields the host code leaves unset are masked).  Pointers are made-up addresses; nothing is dereferenced.  Two builds of
// the library dispatch alike exactly when their outputs are equal (diff).  Where the library exports the route queries
// (hdmoe_conv_fwd_route, hdmoe_conv_wgrad_route) every forward and weight-gradient launch is checked against them; the summary goes to stderr.
#include <cxxabi.h>
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

std::map<const void*, std::string>& kernel_names() { static std::map<const void*, std::string> m; return m; }
std::map<std::string, long> g_count;
std::vector<std::string> g_call;          // kernels launched by the current call
long g_call_no = 0, g_launches = 0;

struct Mask { int lo, hi; };
struct ArgSpec { const char* prefix; std::vector<int> sizes; std::vector<Mask> masks; };   // masks: byte ranges of the first argument
// argument sizes of the kernels under test (the structs are private to their files); others are recorded without kernarg bytes
const ArgSpec kSpecs[] = {
    {"conv_fwd_kernel", {240}, {}},
    {"conv_fwd2_kernel", {240, 4, 4, 4, 4}, {}},
    {"conv_fwd3_kernel", {240, 4, 4, 4, 4, 4}, {}},
    {"conv_fwd5_kernel", {240, 4, 4, 4, 4, 4, 4}, {}},
    {"conv_wgrad_kernel", {276}, {}},
    {"conv_wgrad2_kernel", {276, 64}, {{132, 144}}},          // spw / ob_count / ib_count belong to conv_wgrad_kernel
    {"lwg_", {120}, {{108, 112}}},
    {"swg_f32_kernel", {64}, {}},
    {"towg_bf16_kernel", {64}, {}},
    {"pw_bwd_kernel", {148}, {{124, 128}}},
    {"kgemm_kernel", {56}, {}},
    {"glin_f32_kernel", {76}, {}},
    {"rowlin_f32_kernel", {88}, {}},
};

std::string short_name(const void* f) {
  auto it = kernel_names().find(f);
  if (it == kernel_names().end()) return "?";
  std::string m = it->second;
  for (size_t p; (p = m.find("DF16b")) != std::string::npos;) m.replace(p, 5, "u6__bf16");   // (older demanglers do not know __bf16's code)
  int st = 0;
  char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &st);
  std::string s = st == 0 && d ? d : m;
  free(d);
  const std::string anon = "(anonymous namespace)::";
  size_t p = s.find(anon);
  if (p != std::string::npos) s = s.substr(p + anon.size());
  else if (s.rfind("void ", 0) == 0) s = s.substr(5);
  int depth = 0;
  for (size_t i = 0; i < s.size(); ++i) {               // cut the parameter list
    if (s[i] == '<') ++depth; else if (s[i] == '>') --depth;
    else if (s[i] == '(' && depth == 0) { s.resize(i); break; }
  }
  return s;
}

}  // namespace

extern "C" {

void __hipRegisterFunction(void** modules, const void* host_fn, char* device_fn, const char* device_name, unsigned threads, void* tid, void* bid,
                           dim3* block_dim, dim3* grid_dim, int* w_size) {
  kernel_names()[host_fn] = device_name;
  using Fn = void (*)(void**, const void*, char*, const char*, unsigned, void*, void*, dim3*, dim3*, int*);
  static Fn next = (Fn)dlsym(RTLD_NEXT, "__hipRegisterFunction");
  if (next) next(modules, host_fn, device_fn, device_name, threads, tid, bid, block_dim, grid_dim, w_size);
}

hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
  const std::string name = short_name(f);
  unsigned long long h = 1469598103934665603ull;
  int nbytes = 0;
  for (const ArgSpec& sp : kSpecs) {
    if (name.rfind(sp.prefix, 0) != 0) continue;
    for (size_t i = 0; i < sp.sizes.size(); ++i) {
      std::vector<unsigned char> b((const unsigned char*)args[i], (const unsigned char*)args[i] + sp.sizes[i]);
      if (i == 0) for (const Mask& m : sp.masks) memset(b.data() + m.lo, 0, m.hi - m.lo);
      if (i == 1 && sp.sizes[i] == 64) {                // Wg2Geom: groups[] past ngr are unset
        int ngr; memcpy(&ngr, b.data() + 28, 4);
        memset(b.data() + 32 + 4 * ngr, 0, 4 * (8 - ngr));
      }
      for (unsigned char c : b) { h ^= c; h *= 1099511628211ull; }
      nbytes += sp.sizes[i];
    }
    break;
  }
  printf("%ld %s grid %u %u %u block %u lds %zu args %d %016llx\n", g_call_no, name.c_str(), grid.x, grid.y, grid.z, block.x, lds, nbytes, h);
  ++g_count[name]; ++g_launches;
  g_call.push_back(name);
  return hipSuccess;
}
// kernel<<<...>>> = push the launch configuration, then call the kernel's host stub, which pops it and calls hipLaunchKernel
static struct { dim3 grid, block; size_t lds; hipStream_t stream; } g_config;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) { g_config = {grid, block, lds, stream}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  *grid = g_config.grid; *block = g_config.block; *lds = g_config.lds; *stream = g_config.stream;
  return hipSuccess;
}
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }

}  // extern "C"

namespace {

using FwdFn = int (*)(const void*, const void*, void*, const void*, float, float, const int*, int, long, int, int, int, int, int, int, int, int, int,
                      int, int, int, const int*, const int*, const int*, const int*, int, hipStream_t);
using WgradFn = int (*)(const void*, const void*, float* const*, const int*, int, int, int, int, int, int, int, int, int, int, int, const int*,
                        const int*, const int*, const int*, int, hipStream_t);
using PwFn = int (*)(const void*, const void*, const void*, void*, float* const*, const int*, int, long, int, long, int, int, float, int, hipStream_t);
using FwdRouteFn = int (*)(int*, int, int, int, int, int, int, int, int, int, int, int, int, int, int, int, long, const int*, const int*, const int*, const int*,
                           int, int);
using WgRouteFn = int (*)(int*, int, int, int, int, int, int, int, int, int, int, int, int, const int*, const int*, const int*, const int*, int, int);

FwdFn conv_fwd; WgradFn conv_wgrad; PwFn pw_bwd; FwdRouteFn fwd_route; WgRouteFn wg_route;
long g_route_checked = 0, g_route_bad = 0;

struct Groups { int n; int kh[8], kw[8]; };
const Groups kGroups[] = {
    {1, {1}, {1}}, {1, {2}, {2}}, {1, {3}, {3}}, {1, {4}, {4}}, {1, {5}, {5}}, {1, {7}, {7}}, {1, {1}, {7}}, {1, {3}, {5}},
    {3, {3, 5, 3}, {3, 5, 3}}, {3, {1, 1, 1}, {1, 1, 1}}, {3, {7, 3, 5}, {7, 3, 5}}, {3, {2, 4, 1}, {2, 4, 1}},
    {8, {3, 5, 7, 3, 5, 7, 3, 5}, {3, 5, 7, 3, 5, 7, 3, 5}}, {8, {1, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}},
    {8, {1, 2, 3, 4, 5, 7, 3, 5}, {1, 2, 3, 4, 5, 7, 5, 3}},
};
const int kHW[][2] = {{1, 1}, {4, 4}, {5, 5}, {8, 8}, {16, 16}, {20, 20}, {32, 32}, {64, 64}, {96, 96}, {8, 64}, {1, 64}, {16, 96}, {5, 32}};
const char* tname(int dtype) { return dtype == 0 ? "float" : "__bf16"; }
const char* bname(int v) { return v ? "true" : "false"; }

void check(const std::string& want) {
  ++g_route_checked;
  for (const std::string& got : g_call)
    if (got != want) { ++g_route_bad; fprintf(stderr, "call %ld: route says %s, launched %s\n", g_call_no, want.c_str(), got.c_str()); return; }
}

void run_fwd(int dtype, int stride, int ones, const Groups& g, int N, int H, int W, int Cphys, int Cout, int Cstore, int align) {
  const int Cin = Cphys + ones, Ipad = (Cin + 15) / 16 * 16, Ho = stride ? (H + stride - 1) / stride : H, Wo = stride ? (W + stride - 1) / stride : W;
  int pt[8], pl[8];
  for (int i = 0; i < g.n; ++i) { pt[i] = (g.kh[i] - 1) / 2; pl[i] = (g.kw[i] - 1) / 2; }
  const uintptr_t base = 0x10000000;
  const void* x = (const void*)(base + (align == 1 ? 4 : 0));
  void* y = (void*)(base + 0x1000000 + (align == 2 ? 4 : 0));
  const void* w = (const void*)(base + 0x2000000 + (align == 3 ? 4 : 0));
  const void* res = align == 4 ? nullptr : (const void*)(base + 0x3000000 + (align == 2 ? 4 : 0));
  const int* seg = g.n > 1 ? (const int*)(base + 0x4000000) : nullptr;
  ++g_call_no; g_call.clear();
  const long wstride = (long)49 * Cout * Ipad;
  const int rc = conv_fwd(x, w, y, res, 0.5f, res ? 0.25f : 0.f, seg, g.n, wstride, N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout, Cstore, stride, ones, g.kh,
                          g.kw, pt, pl, dtype, nullptr);
  printf("%ld fwd rc %d\n", g_call_no, rc);
  if (!fwd_route || (align != 0 && align != 4)) return;
  int r[5];
  const int rq = fwd_route(r, N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout, Cstore, stride, ones, g.n, seg != nullptr, res != nullptr, wstride, g.kh, g.kw, pt,
                           pl, dtype, 1);
  if (rc < 0 || rq != 0) {                                  // a refused call: the query refuses it too, or answers "none" (route 9)
    ++g_route_checked;
    if (rc >= 0 || (rq == 0 && r[0] != 9)) { ++g_route_bad; fprintf(stderr, "call %ld: rc %d, route query %d\n", g_call_no, rc, rq); }
    return;
  }
  char buf[128] = "";
  switch (r[0]) {                                           // HDMOE_ROUTE_CONV_*
    case 0: snprintf(buf, sizeof buf, "conv_fwd_kernel<%s, %d, %s>", tname(dtype), r[1], bname(r[2])); break;
    case 1: snprintf(buf, sizeof buf, "conv_fwd2_kernel<%s, %d, %s>", tname(dtype), r[1], bname(r[2])); break;
    case 2: snprintf(buf, sizeof buf, "conv_fwd3_kernel<%s, %d>", tname(dtype), r[1]); break;
    case 3: snprintf(buf, sizeof buf, "conv_fwd5_kernel<%s, %d, %s, %d>", tname(dtype), r[1], bname(r[3]), r[4]); break;
    case 4: snprintf(buf, sizeof buf, "conv7_kernel<%d, %d, %s, false>", r[1], r[2], bname(r[3])); break;
    case 5: snprintf(buf, sizeof buf, "conv6_bf16_kernel<%d, %d, false>", r[1], r[2]); break;
    case 6: snprintf(buf, sizeof buf, "conv6_split_kernel<%d>", r[1]); break;
    case 7: snprintf(buf, sizeof buf, "kgemm_kernel<%d>", r[1]); break;
    case 8: snprintf(buf, sizeof buf, "glin_f32_kernel<%d>", r[1]); break;
    case 10: snprintf(buf, sizeof buf, "rowlin_f32_kernel"); break;
  }
  if ((r[0] == 9) != g_call.empty()) { ++g_route_checked; ++g_route_bad; fprintf(stderr, "call %ld: route %d, %zu launches\n", g_call_no, r[0], g_call.size()); return; }
  check(buf);                                               // (route 9 = none: nothing launched, nothing to compare)
}

void run_wgrad(int dtype, int stride, int ones, const Groups& g, int N, int H, int W, int Cphys, int Cout, int align) {
  const int Cin = Cphys + ones, Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  int pt[8], pl[8];
  for (int i = 0; i < g.n; ++i) { pt[i] = (g.kh[i] - 1) / 2; pl[i] = (g.kw[i] - 1) / 2; }
  const uintptr_t base = 0x10000000;
  const void* x = (const void*)(base + (align ? 4 : 0));
  const void* dy = (const void*)(base + 0x1000000);
  float* G[8];
  for (int i = 0; i < 8; ++i) G[i] = (float*)(base + 0x2000000 + 0x100000 * i);
  const int* seg = g.n > 1 ? (const int*)(base + 0x4000000) : nullptr;
  ++g_call_no; g_call.clear();
  const int rc = conv_wgrad(x, dy, G, seg, g.n, N, H, W, Ho, Wo, Cin, Cphys, Cout, stride, ones, g.kh, g.kw, pt, pl, dtype, nullptr);
  printf("%ld wgrad rc %d\n", g_call_no, rc);
  if (!wg_route || g_call.empty()) return;
  int r[34];
  if (wg_route(r, N, H, W, Ho, Wo, Cin, Cphys, Cout, stride, ones, g.n, seg != nullptr, g.kh, g.kw, pt, pl, dtype, align == 0) != 0) { ++g_route_bad; return; }
  const char* fam[] = {"conv_wgrad2_kernel", "conv_wgrad_kernel<", "swg_f32_kernel", "towg_bf16_kernel", "lwg_"};
  if (r[0] != 0) {
    ++g_route_checked;
    if (g_call[0].rfind(fam[r[0]], 0) != 0) { ++g_route_bad; fprintf(stderr, "call %ld: route %d, launched %s\n", g_call_no, r[0], g_call[0].c_str()); }
    return;
  }
  std::vector<std::string> want;
  for (int k = 0; k < r[1]; ++k)
    for (int p = 0; p < r[2 + 4 * k]; ++p) {
      char buf[128];
      snprintf(buf, sizeof buf, "conv_wgrad2_kernel<%s, %d, %d, %s>", tname(dtype), r[4 + 4 * k], r[3 + 4 * k], bname(r[5 + 4 * k]));
      want.push_back(buf);
    }
  ++g_route_checked;
  if (want != g_call) { ++g_route_bad; fprintf(stderr, "call %ld: wgrad route disagrees (%zu launches)\n", g_call_no, g_call.size()); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s libhdmoe_hip.so\n", argv[0]); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  conv_fwd = (FwdFn)dlsym(lib, "hdmoe_conv_fwd"); conv_wgrad = (WgradFn)dlsym(lib, "hdmoe_conv_wgrad"); pw_bwd = (PwFn)dlsym(lib, "hdmoe_pw_bwd");
  fwd_route = (FwdRouteFn)dlsym(lib, "hdmoe_conv_fwd_route"); wg_route = (WgRouteFn)dlsym(lib, "hdmoe_conv_wgrad_route");
  if (!conv_fwd || !conv_wgrad || !pw_bwd) { fprintf(stderr, "entry points missing\n"); return 2; }
  const int cins[] = {3, 6, 8, 32, 48, 64, 96}, couts[] = {1, 4, 6, 8, 32, 48, 64, 72, 128};
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int stride = 1; stride <= 2; ++stride)
      for (int ones = 0; ones < 2; ++ones)
        for (const Groups& g : kGroups)
          for (const auto& hw : kHW)
            for (int cin : cins)
              for (int cout : couts) {
                for (int align = 0; align < 5; ++align) run_fwd(dtype, stride, ones, g, 2, hw[0], hw[1], cin, cout, cout, align);
                if (cout > 4) run_fwd(dtype, stride, ones, g, 3, hw[0], hw[1], cin, cout, cout - 2, 0);    // stored channels < computed
                for (int align = 0; align < 2; ++align) run_wgrad(dtype, stride, ones, g, 2, hw[0], hw[1], cin, cout, align);
              }
  // more rows than one launch of the row-per-blockIdx.y kernels covers; long contractions (kgemm, glin); the split dtype; refused calls
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int cin : {6, 8})
      for (int cout : {6, 8, 48}) {
        run_fwd(dtype, 1, 0, kGroups[2], 70000, 8, 8, cin, cout, cout, 0);
        run_fwd(dtype, 1, 0, kGroups[2], 70000, 4, 4, cin, cout, cout, 0);
        run_fwd(dtype, 2, 0, kGroups[2], 140000, 8, 8, cin, cout, cout, 0);
      }
  for (int dtype = 0; dtype < 2; ++dtype)
    for (int cin : {256, 512, 768, 1024, 2048})
      for (int cout : {32, 64, 96})
        for (const Groups& g : {kGroups[0], kGroups[9]})
          for (const auto& hw : {kHW[0], kHW[3], kHW[6]}) {
            for (int align : {0, 1}) run_fwd(dtype, 1, 0, g, 64, hw[0], hw[1], cin, cout, cout, align);
            run_wgrad(dtype, 1, 0, g, 64, hw[0], hw[1], cin, cout, 0);
          }
  run_fwd(1, 1, 0, kGroups[5], 2, 8, 64, 8, 36, 36, 0);          // conv_fwd5<bf16, 2, false, 9>: 7x7 block tiles, Cstore % 8 != 0
  for (int cin : {32, 64}) for (int cout : {32, 64}) run_fwd(2, 1, 0, kGroups[2], 2, 32, 32, cin, cout, cout, 0);
  for (int n : {191, 192}) for (int hw : {16, 32}) for (int cout : {32, 64}) for (const Groups& g : {kGroups[8], kGroups[12]})   // conv7 and just below it
    run_fwd(1, 1, 0, g, n, hw, hw, 32, cout, cout, 0);
  run_fwd(7, 1, 0, kGroups[2], 2, 8, 8, 8, 8, 8, 0);
  run_fwd(0, 1, 0, kGroups[2], 2, 8, 8, 8, 8, 16, 0);            // Cstore > Cout
  run_fwd(0, 0, 0, kGroups[2], 2, 8, 8, 8, 8, 8, 0);             // stride 0
  run_fwd(0, 1, 0, kGroups[2], 0, 8, 8, 8, 8, 8, 0);             // empty batch
  { Groups bad = kGroups[2]; bad.n = 9; run_fwd(0, 1, 0, bad, 2, 8, 8, 8, 8, 8, 0); run_wgrad(0, 1, 0, bad, 2, 8, 8, 8, 8, 0); }
  run_wgrad(7, 1, 0, kGroups[2], 2, 8, 8, 16, 8, 0);
  // the fused pointwise backward (pbwd.hip): every channel-tile pair and the refused ones
  for (int cin : {32, 64, 96, 128, 160})
    for (int cout : {32, 64, 96, 128})
      for (int ng : {1, 3})
        for (long hw : {1l, 256l, 4096l}) {
          const uintptr_t base = 0x10000000;
          float* G[8];
          for (int i = 0; i < 8; ++i) G[i] = (float*)(base + 0x2000000 + 0x100000 * i);
          ++g_call_no; g_call.clear();
          const int rc = pw_bwd((const void*)base, (const void*)(base + 0x100000), (const void*)(base + 0x200000), (void*)(base + 0x300000), G,
                                ng > 1 ? (const int*)(base + 0x400000) : nullptr, ng, (long)cin * cout, 16, hw, cin, cout, 0.5f, 1, nullptr);
          printf("%ld pw_bwd rc %d\n", g_call_no, rc);
        }
  fprintf(stderr, "%ld calls, %ld launches, %zu kernel instantiations; route queries: %ld checked, %ld disagree\n", g_call_no, g_launches,
          g_count.size(), g_route_checked, g_route_bad);
  for (const auto& kv : g_count) fprintf(stderr, "%8ld  %s\n", kv.second, kv.first.c_str());
  return g_route_bad ? 1 : 0;
}
