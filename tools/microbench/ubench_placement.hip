// Microbenchmark: where the dispatcher puts the waves of a workgroup.  Every wave stamps its HW_ID register (SIMD, CU, SH, SE)
// and its XCC id into a buffer, then stays resident for ~30 us so that all waves of the launch (or of two concurrent launches)
// hold their places at the same time.  One launch (or one pair of launches on two streams) per case on an otherwise idle
// chip; nothing waits on anything inside a kernel.
//   build: hipcc --offload-arch=gfx950 -O2 -o ubench_placement ubench_placement.hip
// Questions (DESIGN.md "SIMD roles"): does a 4-wave workgroup always have one wave on each SIMD of its CU, a 16-wave
// workgroup four?  How do the one-wave workgroups of two concurrent launches land on SIMDs?
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

struct Stamp {
  unsigned hw_id, xcc_id;
};

// HW_REG_HW_ID = 4, HW_REG_XCC_ID = 20; the immediate is id | offset << 6 | (size - 1) << 11: all 32 bits of each
__global__ void stamp_waves(Stamp *out, unsigned long long ticks, unsigned *sink)
{
  extern __shared__ char pad[]; // the case's LDS claim, unused
  const unsigned long long t0 = wall_clock64();
  if ((threadIdx.x & 63u) == 0) {
    Stamp s;
    s.hw_id = __builtin_amdgcn_s_getreg(4 | (31 << 11));
    s.xcc_id = __builtin_amdgcn_s_getreg(20 | (31 << 11));
    out[(size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = s;
  }
  unsigned v = threadIdx.x;
  while (wall_clock64() - t0 < ticks) v = v * 1664525u + 1013904223u; // 100 MHz ticks
  if (v == 0x12345678u) *sink = v + (unsigned)(size_t)pad;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static unsigned simd_of(const Stamp &s) { return (s.hw_id >> 4) & 3u; }
// a CU of the chip: XCC, SE (HW_ID 15:13), SH (12), CU (11:8)
static unsigned cu_of(const Stamp &s) { return (s.xcc_id & 15u) << 8 | ((s.hw_id >> 8) & 0xFFu); }

int main()
{
  hipStream_t st[2];
  CK(hipStreamCreateWithFlags(&st[0], hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&st[1], hipStreamNonBlocking));
  unsigned *sink;
  CK(hipMalloc(&sink, 4));
  CK(hipFuncSetAttribute(reinterpret_cast<const void *>(stamp_waves), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const unsigned long long ticks = 3000; // 30 us

  // one case: `launches` concurrent launches (one per stream) of `grid` workgroups of `threads` threads and `lds` bytes
  auto run = [&](const char *name, int launches, unsigned threads, unsigned grid, unsigned lds) -> int {
    const unsigned waves_per_wg = threads / 64, waves = grid * waves_per_wg;
    Stamp *d[2] = {nullptr, nullptr};
    std::vector<Stamp> h[2];
    for (int rep = 0; rep < 2; rep++) { // the first repetition loads the code object and warms the queues
      for (int l = 0; l < launches; l++) {
        if (!d[l]) CK(hipMalloc(&d[l], waves * sizeof(Stamp)));
        CK(hipMemset(d[l], 0xFF, waves * sizeof(Stamp)));
      }
      CK(hipDeviceSynchronize());
      for (int l = 0; l < launches; l++) hipLaunchKernelGGL(stamp_waves, dim3(grid), dim3(threads), lds, st[l], d[l], ticks, sink);
      CK(hipDeviceSynchronize());
    }
    for (int l = 0; l < launches; l++) {
      h[l].resize(waves);
      CK(hipMemcpy(h[l].data(), d[l], waves * sizeof(Stamp), hipMemcpyDeviceToHost));
      CK(hipFree(d[l]));
    }
    // per workgroup: its waves on one CU?  how many waves on its fullest and emptiest SIMD?
    unsigned split_cu = 0, even = 0;
    std::map<unsigned, unsigned> start_simd;               // SIMD of wave 0 -> workgroups
    std::map<std::vector<unsigned>, unsigned> order;       // SIMDs of waves 0..3 -> workgroups
    std::map<unsigned, std::vector<unsigned>> per_cu[2];   // CU -> waves per SIMD, per launch
    std::map<unsigned, unsigned> wgs_on_cu, wgs_on_cu_of[2];
    for (int l = 0; l < launches; l++)
      for (unsigned g = 0; g < grid; g++) {
        unsigned n[4] = {0, 0, 0, 0};
        const Stamp *w = &h[l][(size_t)g * waves_per_wg];
        bool same = true;
        for (unsigned i = 0; i < waves_per_wg; i++) {
          n[simd_of(w[i])]++;
          same = same && cu_of(w[i]) == cu_of(w[0]);
          auto &v = per_cu[l][cu_of(w[i])];
          v.resize(4);
          v[simd_of(w[i])]++;
        }
        split_cu += !same;
        even += *std::max_element(n, n + 4) == *std::min_element(n, n + 4) || waves_per_wg < 4;
        start_simd[simd_of(w[0])]++;
        if (waves_per_wg >= 4) order[{simd_of(w[0]), simd_of(w[1]), simd_of(w[2]), simd_of(w[3])}]++;
        wgs_on_cu[cu_of(w[0])]++;
        wgs_on_cu_of[l][cu_of(w[0])]++;
      }
    printf("%s: %d x %u workgroups of %u threads (%u waves), %u B LDS\n", name, launches, grid, threads, waves_per_wg, lds);
    printf("  workgroups with waves on more than one CU: %u; with the same wave count on every SIMD: %u of %u\n", split_cu, even,
           grid * launches);
    printf("  SIMD of wave 0:");
    for (auto &kv : start_simd) printf(" simd%u x %u", kv.first, kv.second);
    printf("\n");
    if (!order.empty()) {
      printf("  SIMDs of waves 0-3:");
      for (auto &kv : order) printf(" %u%u%u%u x %u", kv.first[0], kv.first[1], kv.first[2], kv.first[3], kv.second);
      printf("\n");
    }
    unsigned hist_wg[9] = {0};
    for (auto &kv : wgs_on_cu) hist_wg[std::min(kv.second, 8u)]++;
    printf("  CUs used: %zu; CUs by workgroups on them:", wgs_on_cu.size());
    for (unsigned i = 1; i < 9; i++)
      if (hist_wg[i]) printf(" %u wg x %u", i, hist_wg[i]);
    unsigned same_launch = 0; // CUs that hold two or more workgroups of ONE launch
    for (int l = 0; l < launches; l++)
      for (auto &kv : wgs_on_cu_of[l]) same_launch += kv.second > 1;
    printf("; CUs with several workgroups of one launch: %u\n", same_launch);
    // SIMDs by the waves they hold (both launches together), and SIMDs that hold waves of BOTH launches
    std::map<unsigned, std::vector<unsigned>> all;
    unsigned both = 0;
    for (int l = 0; l < launches; l++)
      for (auto &kv : per_cu[l]) {
        auto &v = all[kv.first];
        v.resize(4);
        for (int s = 0; s < 4; s++) v[s] += kv.second[s];
      }
    if (launches == 2)
      for (auto &kv : per_cu[0]) {
        auto it = per_cu[1].find(kv.first);
        if (it == per_cu[1].end()) continue;
        for (int s = 0; s < 4; s++) both += kv.second[s] && it->second[s];
      }
    std::map<unsigned, unsigned> hist;
    for (auto &kv : all)
      for (int s = 0; s < 4; s++) hist[kv.second[s]]++;
    printf("  SIMDs (of the CUs used) by waves held:");
    for (auto &kv : hist) printf(" %u waves x %u", kv.first, kv.second);
    if (launches == 2) printf("; SIMDs holding waves of both launches: %u", both);
    printf("\n");
    return 0;
  };

  const unsigned enc_lds = 36 * 1024; // the quad encoder's table image
  if (run("4-wave workgroups", 1, 256, 125, 0)) return 1;
  if (run("4-wave workgroups", 1, 256, 250, 0)) return 1;
  if (run("16-wave workgroups", 1, 1024, 125, 0)) return 1;
  if (run("16-wave workgroups", 1, 1024, 250, 0)) return 1;
  if (run("one-wave workgroups, one launch", 1, 64, 125, enc_lds)) return 1;
  if (run("one-wave workgroups, two concurrent launches", 2, 64, 125, enc_lds)) return 1;
  if (run("one-wave workgroups, two concurrent launches", 2, 64, 250, enc_lds)) return 1;
  if (run("4-wave workgroups with the encoder's LDS, two concurrent launches", 2, 256, 125, enc_lds)) return 1;
  if (run("16-wave workgroups with 132 KB of LDS, two concurrent launches", 2, 1024, 125, 132 * 1024)) return 1;
  if (run("16-wave workgroups with 63 KB of LDS, two concurrent launches", 2, 1024, 125, 63 * 1024)) return 1;
  return 0;
}
