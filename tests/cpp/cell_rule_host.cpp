// The rule for one scenario cell (msckf_mono_amd/csrc/host_lists.h, cell_refusal) on its own: no HIP header, a host compiler only.
#include <cstdio>
#include <cstring>

#include "../../msckf_mono_amd/csrc/host_lists.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

int main() {
  using namespace msckf_lists;
  const int K = 33;
  for (int k = 0; k <= K; ++k) CHECK(cell_refusal(k, K, 5, 1, 0) == nullptr);
  CHECK(cell_refusal(0, K, 0, 0, 0) == nullptr);                 // no samples, not skipped: the frame only augments
  CHECK(cell_refusal(0, K, 0, 0, CELL_SKIP) == nullptr);
  const char* why = cell_refusal(K + 1, K, 0, 0, 0);
  CHECK(why && std::strstr(why, "exceeds"));
  why = cell_refusal(-1, K, 0, 0, 0);
  CHECK(why && std::strstr(why, "negative"));
  for (int flags : {2, 4, 3, -1, 1 << 30}) { why = cell_refusal(1, K, 0, 0, flags); CHECK(why && std::strstr(why, "flag")); }
  why = cell_refusal(1, K, 0, 0, CELL_SKIP); CHECK(why && std::strstr(why, "skipped"));
  why = cell_refusal(0, K, 1, 0, CELL_SKIP); CHECK(why && std::strstr(why, "skipped"));
  why = cell_refusal(0, K, 0, 1, CELL_SKIP); CHECK(why && std::strstr(why, "skipped"));
  if (failures) return 1;
  std::printf("cell rule ok\n");
  return 0;
}
