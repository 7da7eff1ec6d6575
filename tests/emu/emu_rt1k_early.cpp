// emu_rt1k_early.cpp — the host emulation (emu.cpp, included whole) compiled with MI355_RT1K_EARLY_B=1, for tests/test_emu_rt1k_early.py.
//
// TEST INFRASTRUCTURE ONLY.  plan.hpp ships the macro at 0 (measured, not the default), so the emulation library the other tests load does not hold
// the head's hand-off protocol of kern_xcd.hpp; this unit does, and adds one entry point that runs a planned c2c transform the way emu_run_plan
// does and hands back the group barrier line of the control block as the fused launch left it.  Built by rt1k_early.mk into
// libmi355emu_early.so (with plan.cpp under the same definition).
#ifndef MI355_RT1K_EARLY_B
#define MI355_RT1K_EARLY_B 1
#endif
#include "emu.cpp"

extern "C" {

// Plans `desc` under the MI355_EMU_* switches this test sets (MI355_EMU_CUS, _XCDS, _XCD_FUSED, _XCD_HX, _XCD_SPLIT, _XCD_SLOTS), runs it out of place on a
// zero-filled workspace, and copies the 16 words of group line `gslot` of XcdCtl::bar into bar_words: [0] A | B barrier, [1] slot re-use, [2] head counter.
// Returns the planner status or 100+ as emu_run_plan_ex does; 105: the plan launched no fused kernel.
int emu_rt1k_early_run(const mi355fft_plan_desc* desc, void* input, uint64_t input_bytes, void* output, uint64_t output_bytes, unsigned gslot,
                       unsigned* bar_words, char* err, size_t err_bytes, char* route, size_t route_bytes, int* launches) {
  using namespace mi355;
  PlannerOptions opt;
  opt.compute_units = std::getenv("MI355_EMU_CUS") ? std::atoi(std::getenv("MI355_EMU_CUS")) : 2;
  opt.xcd_fused = std::getenv("MI355_EMU_XCD_FUSED") ? std::atoi(std::getenv("MI355_EMU_XCD_FUSED")) : 0;
  if (const char* e = std::getenv("MI355_EMU_XCD_SPLIT")) opt.xcd_split = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_SLOTS")) opt.xcd_slots = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_HX")) opt.xcd_hx = std::atoi(e);
  emu::g_xcds = std::getenv("MI355_EMU_XCDS") ? (unsigned)std::atoi(std::getenv("MI355_EMU_XCDS")) : 2u;
  PlanIR ir;
  std::string e;
  if (const int rc = build_plan(*desc, opt, ir, e)) { std::snprintf(err, err_bytes, "%s", e.c_str()); return rc; }
  std::snprintf(route, route_bytes, "%s", ir.route.c_str());
  *launches = (int)ir.steps.size();
  if (desc->in_place || gslot >= 512u) { std::snprintf(err, err_bytes, "out-of-place plans and group lines below 512 only"); return 100; }
  if (input_bytes < ir.in_bytes || output_bytes < ir.out_bytes) { std::snprintf(err, err_bytes, "buffer too small: need %llu in, %llu out", (unsigned long long)ir.in_bytes, (unsigned long long)ir.out_bytes); return 101; }
  std::vector<char> work(ir.work_bytes + 256, 0);
  void* base[5] = {input, output, work.data(), nullptr, ir.table.data()};
  EmuLauncher l;
  const XcdCtl* ctl = nullptr;
  auto lines_fn = [&](int family, int id, const LineArgs& a, unsigned grid) -> bool {
    switch (family) {
      case FAM_ROW_SMALL: return launch_lines_family<FAM_ROW_SMALL>(id, a, grid, l);
      case FAM_ROW_1K: return launch_lines_family<FAM_ROW_1K>(id, a, grid, l);
      case FAM_ROW_BIG: return launch_lines_family<FAM_ROW_BIG>(id, a, grid, l);
      case FAM_PASS_A: return launch_lines_family<FAM_PASS_A>(id, a, grid, l);
      case FAM_PASS_B: return launch_lines_family<FAM_PASS_B>(id, a, grid, l);
    }
    return false;
  };
  for (const Step& s : ir.steps) {
    void* ptr[5];
    for (int i = 0; i < 5; ++i) ptr[i] = s.p[i].buf == BUF_NONE ? nullptr : (char*)base[s.p[i].buf] + s.p[i].off;
    auto xcd_fn = [&](int id, const XcdFusedArgs& a, unsigned grid) { ctl = a.ctl; return launch_xcd_fused(id, a, grid, l); };
    if (!dispatch_step(s, ptr, l, lines_fn, xcd_fn)) { std::snprintf(err, err_bytes, "no kernel for step kind %d variant %d", (int)s.kind, s.variant); return 103; }
  }
  if (l.sticky) { std::snprintf(err, err_bytes, "XCD-fused kernel gave up waiting (sticky=%u)", l.sticky); return 104; }
  if (!ctl) { std::snprintf(err, err_bytes, "the plan launched no fused kernel"); return 105; }
  std::memcpy(bar_words, ctl->bar[gslot], sizeof ctl->bar[gslot]);
  return 0;
}

}  // extern "C"
