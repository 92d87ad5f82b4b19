// Host-only check of tostore_amd/csrc/tsh_scan_widths.h: which tile-scan instantiation a row width takes, which widths
// the fp16 and int8 families serve, and -- argv[1]: tests/golden/scan_width_sweep.json, the widths
// tests/test_gpu_scan_widths.py runs -- that those widths reach every (family, chunk count, kind of row) that any
// width from 1 to 4096 can reach.  A chunk count added to SCAN_NCH_OPTS, or a family's widest row moved, makes the
// reachable set larger than the sweep's: this test then fails until the list follows.
// Prints "scan widths ok"; exit status 1 on a miss.
#include <cctype>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "../../tostore_amd/csrc/tsh_scan_widths.h"

using namespace tsh;

static int fails = 0;
#define CHECK(cond, ...)      \
  do {                        \
    if (!(cond)) {            \
      printf("MISS: ");       \
      printf(__VA_ARGS__);    \
      printf("\n");           \
      ++fails;                \
    }                         \
  } while (0)

enum Family { F32 = 0, F16 = 1, I8 = 2 };
// the kind of row an instantiation meets: d4 == 64 NCH; a row that ends inside its last chunk; one that leaves a whole
// chunk of the kernel's empty as well; a packed-row width (ld = 32 / 64 / 128: the f32 scan's packed kernel, the int8
// tile scan on 8 / 16 / 32 lanes)
enum Kind { FULL = 0, RAGGED = 1, EMPTY_CHUNK = 2, NARROW_32 = 3, NARROW_64 = 4, NARROW_128 = 5 };
static const char *FAMILY[3] = {"f32", "fp16", "int8"};
static const char *KIND[6] = {"full", "ragged", "empty chunk", "ld 32", "ld 64", "ld 128"};
typedef std::tuple<int, int, int> Inst;  // family, nch, kind

static void reach(int d, std::set<Inst> *out) {
  const int ld = (d + 3) / 4 * 4, d4 = ld / 4;
  const int nch = pick_nch(d4);
  if (nch < 0) return;
  const int need = (d4 + 63) / 64;
  int kind = d4 == nch * 64 ? FULL : (need < nch ? EMPTY_CHUNK : RAGGED);
  if (scan_packed_ld(ld)) kind = ld == 32 ? NARROW_32 : (ld == 64 ? NARROW_64 : NARROW_128);
  if (nch <= SCAN_F32_MAX_NCH) out->insert(Inst(F32, nch, kind));
  if (scan_f16_supported(nch, d)) out->insert(Inst(F16, nch, kind));
  if (scan_i8_supported(nch)) out->insert(Inst(I8, nch, kind));
}

static bool read_list(const char *path, std::vector<int> *out) {
  FILE *f = fopen(path, "r");
  if (!f) return false;
  int c, v = -1;
  while ((c = fgetc(f)) != EOF) {
    if (isdigit(c)) v = (v < 0 ? 0 : v * 10) + (c - '0');
    else {
      if (v >= 0) out->push_back(v);
      v = -1;
      if (!(c == '[' || c == ']' || c == ',' || isspace(c))) {  // numbers only
        fclose(f);
        return false;
      }
    }
  }
  if (v >= 0) out->push_back(v);
  fclose(f);
  return true;
}

int main(int argc, char **argv) {
  static_assert(SCAN_NCH_OPTS[0] == 1 && SCAN_NCH_OPTS[SCAN_NCH_COUNT - 1] == SCAN_F32_MAX_NCH, "the list's ends");
  static_assert(SCAN_I8_MAX_NCH <= SCAN_F16_MAX_NCH && SCAN_F16_MAX_NCH <= SCAN_F32_MAX_NCH, "the families nest");
  for (int i = 1; i < SCAN_NCH_COUNT; ++i) CHECK(SCAN_NCH_OPTS[i] > SCAN_NCH_OPTS[i - 1], "the list is not ascending at %d", i);

  // pick_nch: monotone, the smallest listed count at or above the need, -1 beyond the widest
  int prev = 0;
  for (int d4 = 1; d4 <= 1024; ++d4) {
    const int need = (d4 + 63) / 64, got = pick_nch(d4);
    CHECK(got >= prev, "pick_nch(%d) = %d after %d", d4, got, prev);
    prev = got;
    int want = -1;
    for (int i = SCAN_NCH_COUNT - 1; i >= 0; --i)
      if (SCAN_NCH_OPTS[i] >= need) want = SCAN_NCH_OPTS[i];
    CHECK(got == want && got >= need, "pick_nch(%d) = %d, the smallest listed count at or above %d is %d", d4, got, need, want);
  }
  CHECK(pick_nch(1) == 1 && pick_nch(64) == 1 && pick_nch(65) == 2 && pick_nch(512) == 8 && pick_nch(513) == 10 &&
            pick_nch(576) == 10 && pick_nch(577) == 10 && pick_nch(641) == 12 && pick_nch(897) == 16 && pick_nch(1024) == 16,
        "pick_nch at the edges of the list");
  CHECK(pick_nch(1025) == -1 && pick_nch(2000) == -1, "pick_nch beyond 16 chunks");

  // the families' predicates at their edges
  auto f16 = [](int d) { return scan_f16_supported(pick_nch((d + 3) / 4), d); };
  auto i8 = [](int d) { return scan_i8_supported(pick_nch((d + 3) / 4)); };
  CHECK(!f16(248) && f16(256) && !f16(260) && f16(264), "fp16 at d = 248 / 256 / 260 / 264");
  CHECK(f16(3584) && f16(3144) && !f16(3592) && !f16(4096), "fp16 at 14 / 16 chunks");
  CHECK(scan_f16_supported(14, 3584) && !scan_f16_supported(16, 4096) && !scan_f16_supported(0, 256), "fp16 by chunk count");
  CHECK(i8(1) && i8(32) && i8(2048) && !i8(2049) && !i8(2052) && !i8(2560), "int8 at 8 / 10 chunks");
  CHECK(scan_i8_supported(8) && !scan_i8_supported(10) && !scan_i8_supported(0) && !scan_i8_supported(-1), "int8 by chunk count");

  // every instantiation any width can reach ...
  std::set<Inst> all, swept;
  for (int d = 1; d <= 4096; ++d) reach(d, &all);
  // (written out: 12 full + 12 ragged + 4 with an empty chunk + 3 packed widths; 11 + 10 + 3; 8 + 8 + 3 narrow)
  int count[3] = {0, 0, 0};
  for (const Inst &i : all) ++count[std::get<0>(i)];
  CHECK(count[F32] == 31 && count[F16] == 24 && count[I8] == 19, "reachable instantiations: %d / %d / %d", count[F32], count[F16], count[I8]);

  // ... is reached by the sweep's widths
  if (argc < 2) {
    printf("usage: scan_widths_test tests/golden/scan_width_sweep.json\n");
    return 1;
  }
  std::vector<int> widths;
  CHECK(read_list(argv[1], &widths) && !widths.empty(), "cannot read a list of numbers from %s", argv[1]);
  std::set<int> pads;  // chunk counts that meet a row with pad elements (d % 4 != 0) inside a tile scan
  bool narrow_pads = false;  // ... and a packed-row width with them
  for (int d : widths) {
    CHECK(d >= 1 && d <= 4096, "width %d", d);
    reach(d, &swept);
    if (d % 4 && !scan_packed_ld((d + 3) / 4 * 4)) pads.insert(pick_nch((d + 3) / 4));
    if (d % 4 && scan_packed_ld((d + 3) / 4 * 4)) narrow_pads = true;
  }
  for (const Inst &i : all)
    CHECK(swept.count(i), "%s, %d chunks, %s: no width of the sweep reaches it", FAMILY[std::get<0>(i)], std::get<1>(i), KIND[std::get<2>(i)]);
  CHECK(swept.size() == all.size(), "the sweep reaches %d instantiations of %d", (int)swept.size(), (int)all.size());
  for (int i = 0; i < SCAN_NCH_COUNT; ++i)
    CHECK(pads.count(SCAN_NCH_OPTS[i]), "%d chunks: no width of the sweep has pad elements", SCAN_NCH_OPTS[i]);
  CHECK(narrow_pads, "no packed-row width of the sweep has pad elements");
  printf("%d widths reach %d of %d instantiations (f32 %d, fp16 %d, int8 %d)\n", (int)widths.size(), (int)swept.size(), (int)all.size(),
         count[F32], count[F16], count[I8]);

  if (fails) return 1;
  printf("scan widths ok\n");
  return 0;
}
