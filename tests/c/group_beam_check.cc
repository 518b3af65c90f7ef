// Drives csrc/gvl_beam.h's GroupBeamState (the host bookkeeping of gvl_group_beam_search) on a CPU: tests/test_group_beam_host_cpu.py replays the candidate lists
// beam.py's group_beam_search saw, group by group, and compares every line.
// stdin:  "k G vocab max_new eos pad length_penalty early num_return"   (eos / pad -1 = none; early 0 False / 1 True / 2 "never"; floating-point fields in any strtod form)
//         then per step one line with G segments "n  v idx lp  v idx lp ..." (n triples of the group: candidate value, LOCAL flat index, processed log-probability;
//         n = 0 for a group beam.py did not process because it was done)
// stdout: per step "step rc d0 d1 .. | parents | tokens" (d = the groups' done flags after the step); after the step that finishes, num_return lines
//         "final score | ids | transition scores"; an error ends the run with "error rc text".
#include "gvl_beam.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

int main() {
  std::string line;
  if (!std::getline(std::cin, line)) return 2;
  std::istringstream cfg(line);
  int k, G, vocab, max_new, eos, pad, early, n_ret; std::string lp;
  if (!(cfg >> k >> G >> vocab >> max_new >> eos >> pad >> lp >> early >> n_ret)) return 2;
  gvl_beam::GroupBeamState gs;
  const int rc0 = gs.init(k, G, vocab, max_new, eos, pad, std::strtod(lp.c_str(), nullptr), early);
  if (rc0 < 0) { std::printf("error %d %s\n", rc0, gvl_beam::status_text(rc0)); return 0; }
  const int N = 2 * gs.s;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::vector<float> vals((size_t)G * N, 0.f), proc((size_t)G * N, 0.f); std::vector<int> idx((size_t)G * N, 0);
    bool any = false;
    for (int g = 0; g < G; ++g) {
      int n;
      if (!(in >> n)) break;
      any = true;
      if (n != 0 && n != N) return 2;
      // n == 0 for a group that is not done: beam.py raised in an earlier group of this step, and so will step() below before it reads this one
      if (n != 0 && gs.group_done(g)) return 3;            // beam.py processed a group this state holds for done
      for (int i = 0; i < n; ++i) {
        std::string v, p;
        if (!(in >> v >> idx[(size_t)g * N + i] >> p)) return 2;
        vals[(size_t)g * N + i] = (float)std::strtod(v.c_str(), nullptr); proc[(size_t)g * N + i] = (float)std::strtod(p.c_str(), nullptr);
      }
    }
    if (!any) continue;
    std::vector<int> parents(k, -7), tokens(k, -7);
    const int rc = gs.step(vals.data(), idx.data(), proc.data(), N, parents.data(), tokens.data());
    if (rc < 0) { std::printf("error %d %s\n", rc, gvl_beam::status_text(rc)); return 0; }
    std::printf("step %d", rc);
    for (int g = 0; g < G; ++g) std::printf(" %d", gs.group_done(g) ? 1 : 0);
    std::printf(" |");
    for (int j = 0; j < k; ++j) std::printf(" %d", parents[j]);
    std::printf(" |");
    for (int j = 0; j < k; ++j) std::printf(" %d", tokens[j]);
    std::printf("\n");
    if (rc == gvl_beam::BEAM_FINISHED) {
      std::vector<std::vector<int>> ids; std::vector<double> score; std::vector<std::vector<float>> ts;
      const int m = gs.finalize_n(n_ret, &ids, &score, &ts);
      for (int r = 0; r < m; ++r) {
        std::printf("final %.17g |", score[r]);
        for (int t : ids[r]) std::printf(" %d", t);
        std::printf(" |");
        for (float t : ts[r]) std::printf(" %.17g", (double)t);
        std::printf("\n");
      }
      return 0;
    }
  }
  return 0;
}
