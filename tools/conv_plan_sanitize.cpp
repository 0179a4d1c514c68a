// csrc/tgsr_conv_plan.h on its own, for the host sanitizers: every form's plan over a sweep of sizes and operand addresses plus the
// degenerate ones - zeros, negatives, INT_MAX, H W at and past each form's limit, grids past 2^31 - 1 workgroups.  Host arithmetic
// only (no launch, no device access; the pointers are made-up addresses that are never read through).  Build and run on any machine
// with hipcc, no GPU needed:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/conv_plan_sanitize.cpp -o conv_plan_sanitize && ./conv_plan_sanitize
// It must end with "ok" and no sanitizer report.
#include <climits>
#include <cstdio>

#include "../tgsr_amd/csrc/tgsr_conv_plan.h"

using namespace tgsr;

int main() {
  const int sizes[] = {INT_MIN, -1, 0, 1, 3, 4, 5, 8, 9, 16, 17, 61, 64, 128, 449, 2051, 1 << 13, (1 << 13) + 1, 1 << 14, (1 << 14) - 1, 1 << 15, 1 << 26,
                       1 << 28, INT_MAX - 1, INT_MAX};
  const int batches[] = {INT_MIN, -1, 0, 1, 2, 3, 16, 1 << 20, INT_MAX};
  const int couts[] = {INT_MIN, -64, 0, 1, 32, 48, 64, 96, 128, 192, INT_MAX - 63, INT_MAX};
  const int cins[] = {INT_MIN, -4, 0, 1, 3, 4, 6, 8, 12, 64, 1 << 20, INT_MAX - 7, INT_MAX};
  const uintptr_t base = (uintptr_t)1 << 24;
  long long calls = 0, ok = 0, einval = 0, eunsup = 0;
  unsigned long long sum = 0;   // a checksum, so that nothing is optimised away (wraps)
  for (int form = -1; form <= TGSR_CONV_FORMS; ++form)
    for (int B : batches)
      for (int H : sizes)
        for (int W : sizes)
          for (int Cout : couts)
            for (int epi = -1; epi <= 2; ++epi)
              for (int stats = 0; stats <= 1; ++stats) {
                const ConvPlan t = conv_tiles(form, B, H, W, Cout, epi, (B ^ H) & 1, stats);
                ++calls;
                sum += (unsigned long long)(t.status + 3) + t.nslots + t.grid.x + t.grid.y + t.tiles_x + t.tiles_y;
                if (t.status != TGSR_OK && (t.nslots || t.tiles_x || t.groups)) { printf("a refused plan is filled\n"); return 1; }
                if (epi < 0 || stats || (H > 17 && H < (1 << 13) && W != H)) continue;   // the operands' side on a thinner grid
                for (int Cin : cins)
                  for (int off = 0; off <= 8; off += 4)
                    for (int which = 0; which < 5; ++which) {
                      auto at = [&](int i, int w) { return reinterpret_cast<float*>(base * i + (which == w ? off : 0)); };
                      const ConvCall c{which == 4 && off == 8 ? nullptr : at(1, 0), (int64_t)Cin * 7 + (which == 0 ? off / 4 : 0), B, Cin, H, W, at(2, 1), Cout,
                                       off == 4 ? nullptr : at(3, -1), off == 4 && which != 3 ? nullptr : at(4, -1),   // (which 3, off 4: shift alone)
                                       (Cin & 1) ? nullptr : at(5, 2), 12 + (which == 2 ? off / 4 : 0), at(6, 3), 12 + (which == 3 ? off / 4 : 0), epi,
                                       (B ^ H) & 1, stats};
                      const ConvPlan p = conv_plan(form, c);
                      ++calls;
                      ok += p.status == TGSR_OK; einval += p.status == TGSR_EINVAL; eunsup += p.status == TGSR_EUNSUPPORTED;
                      sum += (unsigned long long)p.stages + (unsigned long long)p.grid.x * p.grid.y + p.block.x;
                      if (p.status == TGSR_OK && (p.stages < 1 || p.grid.x < 1 || p.grid.y < 1 || p.block.x < 64)) { printf("an accepted plan is empty\n"); return 1; }
                    }
              }
  printf("%lld plans: %lld accepted, %lld TGSR_EINVAL, %lld TGSR_EUNSUPPORTED (checksum %llu)\nok\n", calls, ok, einval, eunsup, sum);
  return ok > 0 && einval > 0 && eunsup > 0 ? 0 : 1;
}
