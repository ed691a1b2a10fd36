// settings_host.cpp -- msckf_mono_amd/csrc/settings.h on its own, with a host compiler (tests/test_settings.py builds and runs
// this, once more under the address and undefined-behaviour sanitizers): the defaults, every variable into its own field and no
// other, the one refusal, and what a copy takes over.  Exit code 0 and "settings ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../msckf_mono_amd/csrc/settings.h"

using namespace msckf_settings;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the defaults, stated here a second time on purpose (the library's documents promise these numbers)
static bool is_default(const Settings& s) {
  return s.nstreams == 1 && s.fuse_prune == 1 && s.overlap_feature == 0 && s.compress_route == -1 && s.small_update == 84 && s.gain_parts == 0 &&
         s.fused_s == 2 && s.feat_pair == 1 && s.cov_update == 0 && s.gate_early == 0 && s.aniso_mode == 0 && s.lit_tol == -1 && s.lit_route == 0 &&
         s.lit_serial == 0 && s.lit_timers == 0 && s.ring == 6 && s.up_mode == 0 && s.test_fail_upload == -1;
}
static void clear_env() { for (const SettingRow& r : SETTINGS_TABLE) if (r.env) unsetenv(r.env); }
static Settings read_env(const char* name, const char* value, bool* ok = nullptr, std::string* err = nullptr) {
  clear_env();
  if (name) setenv(name, value, 1);
  Settings s; std::string e;
  const bool good = settings_from_env(s, e);
  if (ok) *ok = good; else CHECK(good);
  if (err) *err = e;
  clear_env();
  return s;
}
// the number of table fields in which a and b differ
static int differing(const Settings& a, const Settings& b) {
  int n = 0;
  for (const SettingRow& r : SETTINGS_TABLE) n += (r.field && a.*r.field != b.*r.field) || (r.dfield && a.*r.dfield != b.*r.dfield);
  return n;
}

int main() {
  // every member of the record has a row: 18 fields (17 int, 1 double), and the record holds no more than those
  int nfield = 0, nproc = 0;
  for (const SettingRow& r : SETTINGS_TABLE) { nfield += (r.field || r.dfield); nproc += (!r.field && !r.dfield); CHECK(!(r.field && r.dfield)); CHECK(r.field || r.dfield || r.env); }
  CHECK(nfield == 18 && nproc == 3);
  CHECK(sizeof(Settings) == 17 * sizeof(int) + 4 + sizeof(double));   // (4 bytes of padding before the double) a member without a row would grow the record

  CHECK(is_default(Settings()));
  CHECK(is_default(read_env(nullptr, nullptr)));

  // each variable, set to a valid value that is not its default, lands in its own field and in no other
  struct Case { const char* env; const char* text; int Settings::* field; int want; };
  const Case cases[] = {
      {"MSCKF_HIP_FUSE_PRUNE", "0", &Settings::fuse_prune, 0},       {"MSCKF_HIP_SMALL_UPDATE", "30", &Settings::small_update, 30},
      {"MSCKF_HIP_GAIN_PARTS", "4", &Settings::gain_parts, 4},       {"MSCKF_HIP_GAIN_PARTS", "2", &Settings::gain_parts, 2},
      {"MSCKF_HIP_FUSED_S", "0", &Settings::fused_s, 0},             {"MSCKF_HIP_FEATURE_PAIR", "0", &Settings::feat_pair, 0},
      {"MSCKF_HIP_LITERAL_ROUTE", "1", &Settings::lit_route, 1},     {"MSCKF_HIP_LITERAL_SERIAL", "1", &Settings::lit_serial, 1},
      {"MSCKF_HIP_LITERAL_TIMERS", "1", &Settings::lit_timers, 1},   {"MSCKF_HIP_TEST_FAIL_UPLOAD", "11", &Settings::test_fail_upload, 11},
  };
  for (const Case& c : cases) {
    const Settings s = read_env(c.env, c.text);
    CHECK(s.*c.field == c.want);
    CHECK(differing(s, Settings()) == 1);
  }
  // ... and every row with a variable and a field is among the cases
  for (const SettingRow& r : SETTINGS_TABLE) {
    if (!r.env || !r.field) continue;
    bool seen = false;
    for (const Case& c : cases) seen = seen || (!std::strcmp(c.env, r.env) && c.field == r.field);
    CHECK(seen);
  }
  // the process-wide variables belong to no handle
  for (const char* name : {"MSCKF_HIP_ROCTX", "MSCKF_HIP_HOST_THREADS", "MSCKF_HIP_CYCLE_TIMERS"}) CHECK(is_default(read_env(name, "1")));

  // the one check, its message word for word; what atoi makes of a text is what the field gets
  bool ok = true; std::string err;
  read_env("MSCKF_HIP_GAIN_PARTS", "3", &ok, &err);
  CHECK(!ok && err == "MSCKF_HIP_GAIN_PARTS must be 0, 2 or 4");
  CHECK(read_env("MSCKF_HIP_GAIN_PARTS", "0").gain_parts == 0);
  CHECK(read_env("MSCKF_HIP_SMALL_UPDATE", "0").small_update == 0);
  CHECK(read_env("MSCKF_HIP_SMALL_UPDATE", "-5").small_update == -5);
  CHECK(read_env("MSCKF_HIP_FUSE_PRUNE", "7").fuse_prune == 1);
  CHECK(read_env("MSCKF_HIP_FUSE_PRUNE", "off").fuse_prune == 0);   // atoi("off") == 0
  CHECK(read_env("MSCKF_HIP_FUSED_S", "").fused_s == 0);            // set but empty: atoi("") == 0, as before
  CHECK(read_env("MSCKF_HIP_LITERAL_TIMERS", "5").lit_timers == 1);

  // take_over: exactly the fields the table marks; every field of the source differs from the destination's
  Settings src, dst;
  int k = 100;
  for (const SettingRow& r : SETTINGS_TABLE) { if (r.field) src.*r.field = ++k; if (r.dfield) src.*r.dfield = 0.5 + ++k; }
  CHECK(differing(src, dst) == nfield);
  dst.take_over(src);
  int ncopied = 0;
  for (const SettingRow& r : SETTINGS_TABLE) {
    if (!r.field && !r.dfield) continue;
    const Settings fresh;
    const bool from_src = r.field ? dst.*r.field == src.*r.field : dst.*r.dfield == src.*r.dfield;
    const bool untouched = r.field ? dst.*r.field == fresh.*r.field : dst.*r.dfield == fresh.*r.dfield;
    CHECK(r.copied == COPIED ? from_src : untouched);
    ncopied += r.copied == COPIED;
  }
  // which those are: routes and numerics travel, plumbing stays
  CHECK(ncopied == 14);
  CHECK(dst.small_update == src.small_update && dst.feat_pair == src.feat_pair && dst.lit_route == src.lit_route && dst.lit_serial == src.lit_serial);
  CHECK(dst.nstreams == src.nstreams && dst.fuse_prune == src.fuse_prune && dst.overlap_feature == src.overlap_feature && dst.compress_route == src.compress_route);
  CHECK(dst.gain_parts == src.gain_parts && dst.fused_s == src.fused_s && dst.cov_update == src.cov_update && dst.gate_early == src.gate_early);
  CHECK(dst.aniso_mode == src.aniso_mode && dst.lit_tol == src.lit_tol);
  CHECK(dst.ring == 6 && dst.up_mode == 0 && dst.test_fail_upload == -1 && dst.lit_timers == 0);

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("settings ok\n");
  return 0;
}
