// The pruned-state log's host mirror (msckf_mono_amd/csrc/host_lists.h, PrunedFifo) on its own: no HIP header, a host compiler only.
#include <cstdio>
#include <vector>

#include "../../msckf_mono_amd/csrc/host_lists.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)
using V = std::vector<int>;

int main() {
  using namespace msckf_lists;
  const int cap = 4;
  PrunedFifo m;
  std::vector<int> ncam = {2, 0};                  // trajectory 0 starts with two states whose images are unknown
  m.resync(ncam); m.forget(ncam);                  // the log is off: nothing to do, nothing appears
  CHECK(m.fifo.empty() && m.aug.empty());
  m.start(ncam);
  CHECK(m.fifo.size() == 2 && m.aug.size() == 2);
  CHECK(m.fifo[0] == V({-1, -1}) && m.fifo[1].empty() && m.aug[0].empty() && m.aug[1].empty());

  // an augment pushes the ordinal
  m.mirror(0, true, 0, 10, cap); m.mirror(1, true, 0, 10, cap);
  CHECK(m.fifo[0] == V({-1, -1, 10}) && m.fifo[1] == V({10}) && m.aug[0].empty() && m.aug[1].empty());
  // nd == 0 with no augment changes nothing
  m.mirror(0, false, 0, 11, cap); m.mirror(1, false, 0, 11, cap);
  CHECK(m.fifo[0] == V({-1, -1, 10}) && m.fifo[1] == V({10}) && m.aug[0].empty() && m.aug[1].empty());
  // a drop of nd pops the nd oldest into the stored ordinals, in order; the frame's own state can be among them
  m.mirror(0, true, 3, 12, cap);
  CHECK(m.fifo[0] == V({12}) && m.aug[0] == V({-1, -1, 10}));
  m.mirror(1, true, 2, 12, cap);
  CHECK(m.fifo[1].empty() && m.aug[1] == V({10, 12}));
  // stored ordinals stop at the capacity while the FIFO still pops
  m.mirror(0, true, 0, 13, cap); m.mirror(0, true, 0, 14, cap);
  m.mirror(0, true, 3, 15, cap);
  CHECK(m.fifo[0] == V({15}) && m.aug[0] == V({-1, -1, 10, 12}));
  m.mirror(0, false, 1, 16, cap);
  CHECK(m.fifo[0].empty() && m.aug[0].size() == (size_t)cap);

  // a window whose size changed behind the log's back becomes all -1; one that kept its size keeps its ordinals
  m.mirror(0, true, 0, 17, cap); m.mirror(1, true, 0, 17, cap);
  ncam = {3, 1};
  m.resync(ncam);
  CHECK(m.fifo[0] == V({-1, -1, -1}) && m.fifo[1] == V({17}));
  CHECK(m.aug[0].size() == (size_t)cap && m.aug[1] == V({10, 12}));      // the records stay
  // states taken over from another handle: every image unknown, whatever the size
  m.forget(ncam);
  CHECK(m.fifo[0] == V({-1, -1, -1}) && m.fifo[1] == V({-1}) && m.aug[1] == V({10, 12}));
  // reset: no records, the window as it is
  m.start(ncam);
  CHECK(m.fifo[0] == V({-1, -1, -1}) && m.fifo[1] == V({-1}) && m.aug[0].empty() && m.aug[1].empty());
  m.clear();
  CHECK(m.fifo.empty() && m.aug.empty());
  if (failures) return 1;
  std::printf("pruned fifo ok\n");
  return 0;
}
