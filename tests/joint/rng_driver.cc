// Host driver of the normal stream (sparsergps_amd/csrc/sgp_rng.h): the header is HIP-free, so this
// program runs the generator's arithmetic as the kernels run it.
// stdin, one request per line:
//   K c0 c1 c2 c3 k0 k1     (hex words)  -> the four Philox4x32-10 output words, hex
//   N seed stream S n       (decimal)    -> S * n normals, draw-major (all rows of draw 0 first)
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../sparsergps_amd/csrc/sgp_rng.h"

int main() {
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    if (line[0] == 'K') {
      uint32_t c[4], k[2], w[4];
      if (sscanf(line + 1, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32,
                 &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) != 6)
        return 2;
      sgp_philox4x32(c, k, w);
      printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", w[0], w[1], w[2], w[3]);
    } else if (line[0] == 'N') {
      uint64_t seed;
      long long S, n;
      int stream;
      if (sscanf(line + 1, "%" SCNu64 " %d %lld %lld", &seed, &stream, &S, &n) != 4) return 2;
      if (S < 1 || n < 1 || (stream != SGP_RNG_STREAM_JOINT && stream != SGP_RNG_STREAM_ROW))
        return 2;
      for (long long s = 0; s < S; ++s)
        for (long long j = 0; j < n; ++j)
          printf("%.17g\n", stream == SGP_RNG_STREAM_JOINT
                                ? sgp_rng_joint(seed, (uint64_t)s, (uint64_t)j)
                                : sgp_rng_row(seed, (uint64_t)s, (uint64_t)j));
    } else if (line[0] != '\n') {
      return 2;
    }
  }
  return 0;
}
