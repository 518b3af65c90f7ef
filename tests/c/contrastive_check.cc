// contrastive_check.cc -- drives csrc/gvl_contrastive.h (host-only: this file includes nothing else of the library) for tests/test_contrastive_host_cpu.py.
// stdin:  "k max_new eos" then per step "sel id_0 .. id_{k-1} seq_0 .. seq_{k-1}";  stdout per step: "step <status>|<winner>|<losers>", then "ids|<ids>|<ranks>".
// A line "refusal top_k alpha max_new max_new_cap cap vocab hidden" prints "refusal|<text or ->" instead.
#include <cstdio>
#include <cstring>
#include <vector>
#include "gvl_contrastive.h"

int main() {
  char word[32];
  gvl_contrastive::State st;
  bool have = false;
  while (std::scanf("%31s", word) == 1) {
    if (!std::strcmp(word, "refusal")) {
      int k, max_new, max_cap, cap, vocab, hidden; float alpha;
      if (std::scanf("%d %f %d %d %d %d %d", &k, &alpha, &max_new, &max_cap, &cap, &vocab, &hidden) != 7) return 2;
      const char* why = gvl_contrastive::refusal(k, alpha, max_new, max_cap, cap, vocab, hidden);
      std::printf("refusal|%s\n", why ? why : "-");
      continue;
    }
    if (!std::strcmp(word, "init")) {
      int k, max_new, eos;
      if (std::scanf("%d %d %d", &k, &max_new, &eos) != 3) return 2;
      std::printf("init %d\n", st.init(k, max_new, eos));
      have = true;
      continue;
    }
    if (!std::strcmp(word, "step") && have) {
      int sel;
      if (std::scanf("%d", &sel) != 1) return 2;
      std::vector<int> ids(st.k), seqs(st.k), losers(st.k, -1);
      for (int& v : ids) if (std::scanf("%d", &v) != 1) return 2;
      for (int& v : seqs) if (std::scanf("%d", &v) != 1) return 2;
      int winner = -1;
      const int rc = st.step(ids.data(), sel, seqs.data(), &winner, losers.data());
      std::printf("step %d|%d|", rc, winner);
      for (int i = 0; i + 1 < st.k && rc >= 0; ++i) std::printf("%s%d", i ? " " : "", losers[i]);
      std::printf("\n");
      continue;
    }
    if (!std::strcmp(word, "end")) {
      std::printf("ids|");
      for (size_t i = 0; i < st.ids.size(); ++i) std::printf("%s%d", i ? " " : "", st.ids[i]);
      std::printf("|");
      for (size_t i = 0; i < st.ranks.size(); ++i) std::printf("%s%d", i ? " " : "", st.ranks[i]);
      std::printf("|%d\n", st.finished ? 1 : 0);
      continue;
    }
    return 3;
  }
  return 0;
}
