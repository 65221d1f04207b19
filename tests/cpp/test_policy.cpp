// The dog-leg functions of kalibr_amd/csrc/kb_policy.h on the CPU, called in the order a pass calls them.  One case
// per line on stdin:
//   delta J gg ghg have_gn gn2 ggn have_rho rho
// delta: the trust radius the pass starts with; J: the cost L0 is formed with; gg, ghg: g.g and g^T (J^T J) g of the
// system; gn2, ggn: dx_gn.dx_gn and g.dx_gn of its GN step (have_gn: the caller has one to offer; it is held only when
// the SD branch is not taken); rho: the gain ratio the next pass finds (have_rho: there is a next pass).  One line out:
//   sd_branch type delta beta L0 sd_scale dx_sd_norm a b dx_norm radius
// radius: delta after dl_radius(rho), NaN without a next pass.  g++, no HIP.
#include <cmath>
#include <cstdio>

#include "../../kalibr_amd/csrc/kb_policy.h"

int main() {
  double delta, J, gg, ghg, gn2, ggn, rho;
  int have_gn, have_rho;
  while (std::scanf("%lf %lf %lf %lf %d %lf %lf %d %lf", &delta, &J, &gg, &ghg, &have_gn, &gn2, &ggn, &have_rho, &rho) == 9) {
    if (!kb::dl_delta_valid(delta)) return 2;
    kb::KbDl s;
    kb::dl_start(&s, delta);
    kb::dl_set_sd(&s, gg, ghg);
    const bool sd = kb::dl_sd_branch(&s);
    if (!sd) {
      if (!have_gn) return 3;  // the pass needs a GN step the case does not carry
      kb::dl_hold_gn(&s, gn2, ggn);
    }
    kb::dl_select(&s, J);
    const double selected = s.delta;  // the selection sets it in the first step
    double radius = NAN;
    if (have_rho) {
      kb::dl_radius(&s, rho);
      radius = s.delta;
    }
    std::printf("%d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", (int)sd, s.step_type, selected, s.beta,
                s.L0, s.sd_scale, s.dx_sd_norm, s.a, s.b, s.dx_norm, radius);
  }
  return 0;
}
