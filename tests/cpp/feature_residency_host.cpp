// The slot arithmetic of k_feature_pair (msckf_mono_amd/csrc/update_routes.h: PAIR_WAVES_PER_SIMD, feature_pair_residency) as a
// stand-alone host program, for tests/test_feature_residency.py.  One line per window length lm = 2 .. M_REG, then the launch
// of a slice (trajectories x tracks given on the command line) against the slots of the chip at the shipped number of
// wavefronts per SIMD and at one fewer.
//   feature_residency_host TRAJECTORIES TRACKS COMPUTE_UNITS
#include <cstdio>
#include <cstdlib>

#include "../../msckf_mono_amd/csrc/update_routes.h"

int main(int argc, char** argv) {
  using namespace msckf::routes;
  if (argc != 4) { std::fprintf(stderr, "usage: %s trajectories tracks compute_units\n", argv[0]); return 2; }
  const int nb = std::atoi(argv[1]), f_cap = std::atoi(argv[2]), cus = std::atoi(argv[3]);
  std::printf("waves_per_simd=%d simds_per_cu=%d feature_lds=%zu m_reg=%d\n", PAIR_WAVES_PER_SIMD, SIMDS_PER_CU, FEATURE_LDS, M_REG);
  for (int lm = 2; lm <= M_REG; ++lm) {
    const PairResidency r = feature_pair_residency(lm);
    int s_cap = 0;
    const size_t lds = feature_pair_lds_bytes(lm, s_cap);
    std::printf("lm=%d lds=%zu s_cap=%d same_as_launch=%d waves_per_cu=%d lds_fits=%d\n", lm, r.lds_bytes, r.s_cap, (int)(lds == r.lds_bytes && s_cap == r.s_cap),
                r.waves_per_cu, (int)r.lds_fits);
  }
  // the pair launch of this slice, as launch_feature makes it (feat_pair = 1, information form)
  const FeatureRoute fr = feature_route(4, f_cap, M_REG, nb, 1, 3);
  if (fr.n < 1 || !fr.l[0].pair || fr.l[0].single) { std::fprintf(stderr, "not a pair launch\n"); return 1; }
  const long waves = (long)nb * fr.l[0].items;
  for (int w = PAIR_WAVES_PER_SIMD; w >= PAIR_WAVES_PER_SIMD - 1; --w) {
    const PairResidency r = feature_pair_residency(fr.l[0].lm, w);
    std::printf("launch waves_per_simd=%d wavefronts=%ld slots=%ld one_residency=%d\n", w, waves, r.slots(cus), (int)r.one_residency(waves, cus));
  }
  return 0;
}
