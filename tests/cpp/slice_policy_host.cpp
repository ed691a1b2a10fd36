// slice_policy_host.cpp -- msckf_mono_amd/csrc/slice_policy.h on its own, with a host compiler (tests/test_slice_policy.py builds
// and runs this, once more under the address and undefined-behaviour sanitizers): the slice count over the whole grid of
// requests, batches and queue budgets, and what the text of GPU_MAX_HW_QUEUES parses to.  "--table" prints the counts of the
// cases the GPU test asks for.  Exit code 0 and "slice policy ok" when everything holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../msckf_mono_amd/csrc/slice_policy.h"

using namespace msckf::slices;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static int budget_of(const char* text) { return parse_hw_queue_budget(text); }   // the text of GPU_MAX_HW_QUEUES; null: not set

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--table")) {
    // "requested B process_budget streamed : slices", as a handle created under that budget decides
    for (int req : {1, 4})
      for (int B : {1, 3, 8})
        for (int pb : {4, 8})
          for (int streamed = 0; streamed < 2; ++streamed)
            std::printf("%d %d %d %d : %d\n", req, B, pb, streamed, effective_slices(req, B, handle_queue_budget(pb), streamed != 0));
    return 0;
  }
  const int batches[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 64};
  for (int req = 1; req <= SLICES_MAX; ++req)
    for (int B : batches)
      for (int streamed = 0; streamed < 2; ++streamed) {
        const int today = std::max(1, std::min(req, B));   // n_slices() before there was a policy
        int prev = 0;
        for (int budget = 1; budget <= HW_QUEUES_MAX; ++budget) {
          const int n = effective_slices(req, B, budget, streamed != 0);
          CHECK(n >= 1 && n <= std::min(req, B));
          if (budget >= req + streamed) CHECK(n == today);
          CHECK(n >= prev);                                  // monotone in the budget
          prev = n;
          CHECK(effective_slices(req, B, budget, streamed != 0, true) == today);         // msckf_hip_set_slices_exact
          CHECK(effective_slices(req, B, budget, streamed != 0, false, true) == 1);      // stage profiling: one stream
          CHECK(effective_slices(req, B, budget, streamed != 0, true, true) == 1);
        }
      }
  // the table's entries are counts that fit their queues, and never fall as the queues grow
  for (int q = 1; q <= SLICES_MAX; ++q) {
    CHECK(BEST_STREAMED[q] >= 1 && BEST_STREAMED[q] <= q && BEST_STREAMED[q] >= BEST_STREAMED[q - 1]);
    CHECK(BEST_RESIDENT[q] >= 1 && BEST_RESIDENT[q] <= q && BEST_RESIDENT[q] >= BEST_RESIDENT[q - 1]);
  }
  // what the measurement decided (profiles/hw_queue_slices.md): the default of 4 queues runs 2 of 4 requested slices, 8 run all
  CHECK(effective_slices(4, 64, handle_queue_budget(4), true) == 2 && effective_slices(4, 64, handle_queue_budget(4), false) == 2);
  CHECK(effective_slices(4, 64, handle_queue_budget(8), true) == 4 && effective_slices(4, 64, handle_queue_budget(8), false) == 4);
  CHECK(handle_queue_budget(1) == 1 && handle_queue_budget(4) == 3 && handle_queue_budget(32) == 31);

  // GPU_MAX_HW_QUEUES: unset, empty or no number is the runtime's default of 4; a number is clamped to 1 .. 32
  CHECK(HW_QUEUES_DEFAULT == 4 && HW_QUEUES_MAX == 32);
  CHECK(budget_of(nullptr) == 4);
  CHECK(budget_of("") == 4);
  CHECK(budget_of("abc") == 4);
  CHECK(budget_of("0") == 1);
  CHECK(budget_of("-3") == 1);
  CHECK(budget_of("99") == 32);
  CHECK(budget_of("99999999999999999999999") == 32);
  CHECK(budget_of("1") == 1 && budget_of("4") == 4 && budget_of("8") == 8 && budget_of("32") == 32 && budget_of("33") == 32);
  CHECK(budget_of(" 8") == 8 && budget_of("8 ") == 8);   // strtol: leading blanks skipped, a tail ignored

  if (failures) return 1;
  std::printf("slice policy ok\n");
  return 0;
}
