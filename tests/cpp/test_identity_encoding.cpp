// Host-only check of the C++ mirror's base encoding (include/msm_hip.hpp: points_to_bytes): the point at infinity throws by default and is
// written as 64 zero bytes under MSM_HIP_BASES_ZERO_IS_IDENTITY; other points are x || y either way.  Needs no device.
#include <cstdio>

#include "msm_hip.hpp"

using namespace msm_webgpu;

int main() {
  static_assert(MSM_HIP_BASES_ZERO_IS_IDENTITY == 128u, "flag value");
  std::vector<G1Affine> g(3);
  g[0].x[0] = 1;
  g[0].y[0] = 2;
  g[1].infinity = true;
  g[1].x[5] = 7;  // (coordinates of an infinity record are not read)
  g[2].x[31] = 0x11;
  g[2].y[0] = 0x22;
  bool threw = false;
  try {
    (void)points_to_bytes(g);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  if (!threw) {
    std::printf("default encoding accepted the point at infinity\n");
    return 1;
  }
  const std::vector<uint8_t> b = points_to_bytes(g, MSM_HIP_BASES_ZERO_IS_IDENTITY | MSM_HIP_CHECK_ON_CURVE);
  if (b.size() != 3 * 64) return 2;
  for (int k = 64; k < 128; k++)
    if (b[k]) {
      std::printf("infinity record byte %d is %d\n", k, b[k]);
      return 3;
    }
  if (b[0] != 1 || b[32] != 2 || b[128 + 31] != 0x11 || b[128 + 32] != 0x22) return 4;
  g[1].infinity = false;  // without an infinity, both encodings agree
  if (points_to_bytes(g) != points_to_bytes(g, MSM_HIP_BASES_ZERO_IS_IDENTITY)) return 5;
  std::printf("identity encoding ok\n");
  return 0;
}
