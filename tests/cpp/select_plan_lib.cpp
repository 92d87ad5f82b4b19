// The K2 select's plan (tostore_amd/csrc/tsh_select_plan.h, host only) behind C entry points, for the NumPy model of
// the select (tests/select_model.py): the model takes every branch condition from the header the kernel is compiled
// from, through a shared object that g++ builds from this file, and retypes none of them.
#include "../../tostore_amd/csrc/tsh_select_plan.h"

using namespace tsh;

extern "C" {
// out[0..3]: SEL_THREADS, SEL_VPT, SEL_LIST_CAP, SEL_PREFILTER_MIN
void sp_constants(int *out) {
  out[0] = SEL_THREADS;
  out[1] = SEL_VPT;
  out[2] = SEL_LIST_CAP;
  out[3] = SEL_PREFILTER_MIN;
}
int sp_variant(int n_tiles, int k, int has_list) { return (int)select_variant(n_tiles, k, has_list != 0); }
int sp_variant_threads(int v) { return select_variant_threads((SelectVariant)v); }
int sp_variant_in_regs(int v) { return select_variant_in_regs((SelectVariant)v) ? 1 : 0; }
int sp_narrow(int nt, int m, unsigned k, int force_all) { return sel_narrow(nt, m, k, force_all != 0) ? 1 : 0; }
int sp_prefilter(int narrow, int m) { return sel_prefilter(narrow != 0, m) ? 1 : 0; }
int sp_groups4(int nt, unsigned k) { return sel_groups4(nt, k) ? 1 : 0; }
int sp_groups2k(unsigned k) { return sel_groups2k(k) ? 1 : 0; }
int sp_short_small(unsigned n) { return sel_short_small(n) ? 1 : 0; }
int sp_flooded(unsigned n) { return sel_flooded(n) ? 1 : 0; }
int sp_over(unsigned tiles_hit) { return sel_over(tiles_hit) ? 1 : 0; }
int sp_refines(unsigned first_count, int cand_cap) { return sel_refines(first_count, cand_cap) ? 1 : 0; }
int sp_refine_in_regs(int nt, unsigned tiles_hit) { return sel_refine_in_regs(nt, tiles_hit) ? 1 : 0; }
int sp_list_shortcut(int m, unsigned k) { return sel_list_shortcut(m, k) ? 1 : 0; }
int sp_default_entries(int k) { return select_default_entries(k); }
}
