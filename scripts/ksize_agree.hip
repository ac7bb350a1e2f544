// usage: hipcc --offload-arch=gfx950 -I include scripts/ksize_agree.hip -o /tmp/ksize_agree && /tmp/ksize_agree      (host only, no GPU)
// pil_ksize (csrc/pil_resize.h) counts Pillow's taps per output index in integers; data.py's bilinear_table -- and the launchers of
// batch_prep.hip / rgb_prep.hip before they shared the header -- count them in fp64 as Pillow's precompute_coeffs does:
// int(ceil(max(in / out, 1))) * 2 + 1.  This program compares the two wherever a launcher admits the sizes: every in, out in 1..4096
// with in <= 8 out (the two loaders), and every out <= 64 with in <= 4096 (object patches).  Exit status 0: they agree everywhere.
#include <cstdio>
#include "../robocupvision_amd/csrc/pil_resize.h"

static long long ksize_fp64(int in, int out) {
  double scale = (double)in / out;
  if (scale < 1.0) scale = 1.0;
  long long c = (long long)scale;
  if ((double)c < scale) ++c;
  return c * 2 + 1;
}

int main() {
  long long n = 0, bad = 0;
  for (int out = 1; out <= 4096; ++out)
    for (int in = 1; in <= 4096; ++in) {
      if (!(in <= 8 * out || out <= 64)) continue;
      ++n;
      if (pil_ksize(in, out) != ksize_fp64(in, out)) {
        if (++bad <= 10) printf("in %d out %d: integers %lld, fp64 %lld\n", in, out, pil_ksize(in, out), ksize_fp64(in, out));
      }
    }
  printf("%lld pairs, %lld differ\n", n, bad);
  return bad != 0;
}
