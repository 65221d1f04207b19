// Direction probe for the DPP row rotations that k_buildp's SYRK operand fetch relies on: every lane holds its own
// lane id, and the host prints, per control, which lane each lane of row 0 received.  row_ror:n (0x120 + n) delivers
// lane (i - n) & 15 of the same 16-lane row to lane i, so "the value of lane (i + 4) & 15" is row_ror:12.
#include <hip/hip_runtime.h>
#include <cstdio>

template <int CTRL>
__device__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

__global__ void k_probe(int* out) {
  const int lane = threadIdx.x;
  out[lane] = dpp_i<0x124>(lane);
  out[64 + lane] = dpp_i<0x128>(lane);
  out[128 + lane] = dpp_i<0x12C>(lane);
}

int main() {
  int* d;
  if (hipMalloc(&d, sizeof(int) * 192) != hipSuccess) return 1;
  hipLaunchKernelGGL(k_probe, dim3(1), dim3(64), 0, 0, d);
  int h[192];
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  const char* names[3] = {"row_ror:4 ", "row_ror:8 ", "row_ror:12"};
  for (int c = 0; c < 3; ++c) {
    printf("%s lane i <- lane:", names[c]);
    for (int i = 0; i < 64; ++i) printf(" %d", h[64 * c + i]);
    printf("\n");
  }
  hipFree(d);
  return 0;
}
