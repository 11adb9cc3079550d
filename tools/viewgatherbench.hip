// What does the view gather cost per rotation?  64 patches of 448 x 448 are cut out of 64 stored 4480 x 4480 images
// (fp32 and uint8) through image views, per rotation, and compared with (1) gather_kernel on the same patches (the
// yardstick: rot 0 should sit with it) and (2) for 90 / 270 a DIRECT variant that is not shipped: one element per lane
// read at a stride of Ws, the stores coalesced.  The shipped kernel turns a 64 x 64 tile in LDS instead.  Every launch
// takes another set of grid cells, so that the patches do not come out of the 256 MiB Infinity Cache: the 100 cells of
// the 64 images are 15.4 GB (fp32) / 3.85 GB (uint8).  Reports us per launch and GB/s of bytes read plus written.
//   build: hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/viewgatherbench.hip -o tools/viewgatherbench
//   kernel times without the launch gaps: rocprofv3 --kernel-trace --stats -- tools/viewgatherbench
#include "../jolineedle_amd/csrc/kernels_env.hip"
#include "../jolineedle_amd/csrc/kernels_view.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// the variant the shipped kernel has to beat: lanes along the output row, each reading down a source column
template <typename ST>
__global__ __launch_bounds__(256) void direct_turned_kernel(const jn_image_view* __restrict__ views,
                                                            const long long* __restrict__ pos, float* __restrict__ out,
                                                            int P, long long total) {
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int q = (int)(idx % P), r = (int)((idx / P) % P), c = (int)((idx / ((long long)P * P)) % 3);
    const long long n = idx / ((long long)P * P * 3);
    const jn_image_view v = views[n];
    const long long Hr = v.Ws, Wr = v.Hs;
    const long long Y = pos[2 * n] * P + r, X = pos[2 * n + 1] * P + q, y1 = Y - v.ty, x1 = X - v.tx;
    float val = 0.f;
    if (Y < Hr && X < Wr && y1 >= 0 && y1 < Hr && x1 >= 0 && x1 < Wr) {
      const long long srow = v.rot == 90 ? v.Hs - 1 - x1 : x1, scol = v.rot == 90 ? y1 : v.Ws - 1 - y1;
      const ST s = ((const ST*)v.src)[((long long)c * v.Hs + srow) * v.Ws + scol];
      if constexpr (sizeof(ST) == 1) val = jnr::u8_unit(s); else val = s;
    }
    out[idx] = val;
  }
}

template <typename ST>
static void run(const char* name) {
  const int N = 64, W = 4480, P = 448, G = W / P, IT = 10;
  ST* img; float* out; long long* pos; jn_image_view* vt;
  const size_t plane = (size_t)3 * W * W;
  CK(hipMalloc(&img, N * plane * sizeof(ST))); CK(hipMemset(img, 1, N * plane * sizeof(ST)));
  CK(hipMalloc(&out, (size_t)N * 3 * P * P * 4)); CK(hipMalloc(&pos, (size_t)(IT + 2) * N * 2 * 8)); CK(hipMalloc(&vt, N * sizeof(jn_image_view)));
  std::vector<long long> hp((size_t)(IT + 2) * N * 2);
  for (int it = 0; it < IT + 2; ++it)
    for (int i = 0; i < N; ++i) { hp[((size_t)it * N + i) * 2] = (i * 7 + it * 3) % G; hp[((size_t)it * N + i) * 2 + 1] = (i * 3 + it) % G; }
  CK(hipMemcpy(pos, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const double bytes = (double)N * 3 * P * P * (sizeof(ST) + 4.0);
  auto timed = [&](const char* what, auto&& launch) {
    for (int w = 0; w < 2; ++w) launch(pos + (size_t)w * N * 2);
    CK(hipEventRecord(e0));
    for (int it = 0; it < IT; ++it) launch(pos + (size_t)(it + 2) * N * 2);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    printf("%-6s %-28s %8.1f us  %7.0f GB/s\n", name, what, ms * 1e3 / IT, bytes / (ms * 1e-3 / IT) / 1e9);
  };
  timed("gather_kernel (plain)", [&](const long long* p) {
    jnr::launch_gather(img, (const int64_t*)p, out, 3LL * P * P, N, 3, W, W, P, nullptr, 0, nullptr);
  });
  struct V { int rot, ty, tx; const char* what; };
  for (V c : {V{0, 0, 0, "views rot 0"}, V{0, 8, -12, "views rot 0 shift (8,-12)"}, V{0, 3, 5, "views rot 0 shift (3,5)"},
              V{180, 3, 5, "views rot 180 shift (3,5)"}, V{90, 3, 5, "views rot 90 shift (3,5)"}, V{270, 3, 5, "views rot 270 shift (3,5)"}}) {
    std::vector<jn_image_view> hv(N);
    for (int i = 0; i < N; ++i) hv[i] = jn_image_view{img + i * plane, sizeof(ST) == 1, W, W, c.rot, c.ty, c.tx};
    CK(hipMemcpy(vt, hv.data(), N * sizeof(jn_image_view), hipMemcpyHostToDevice));
    timed(c.what, [&](const long long* p) {
      jnr::launch_view_gather(vt, sizeof(ST) == 1, nullptr, (const int64_t*)p, out, 0, 3LL * P * P, N, P, nullptr, 0, nullptr);
    });
    if (c.rot == 90 || c.rot == 270) {
      const long long total = (long long)N * 3 * P * P;
      timed(c.rot == 90 ? "direct strided rot 90" : "direct strided rot 270", [&](const long long* p) {
        hipLaunchKernelGGL((direct_turned_kernel<ST>), dim3(256 * 32), dim3(256), 0, nullptr, vt, p, out, P, total);
      });
    }
  }
  CK(hipFree(img)); CK(hipFree(out)); CK(hipFree(pos)); CK(hipFree(vt));
}

int main() {
  run<float>("fp32");
  run<uint8_t>("uint8");
  return 0;
}
