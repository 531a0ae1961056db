// Error text and version of libmmtta.so.
#include "common.h"
#include <string.h>

namespace mmtta {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int g_profile_main_only = 0;
int g_igemm_pipeline = 1;
int g_epilogue_vec = 1;
int g_igemm_lean = 1;
int g_igemm_reuse = 1;
int g_cls_fused_min = 128;
int g_thin_mfma = 2;
int g_wgrad_vec = 1;
int g_lame_tiled = 1;
int g_raw_staging = 3;
int g_head_loss_pair = 3;
int g_thin_lean = 3;
int g_wgrad_epilogue_update = 1;
int g_cls8_pipeline = 1;
int g_cls8_lean_epilogue = 1;
// split-K below / target, weight-gradient workgroups, thin-layer slabs.  Swept with the lanes bound to their own hardware
// queues (profiles/r02_tuning_sweep.txt): four volumes in flight want half the splitting two did (96/128, 128 slabs)
int g_tune[4] = {96, 128, 128, 256};
}  // namespace mmtta

// How mmtta_set_option stores a value
enum OptKind {
  OPT_AS_IS,       // the value itself
  OPT_FLAG,        // value != 0
  OPT_BIT0,        // value & 1
  OPT_BITS01,      // value & 3
  OPT_0_TO_3,      // clamped to 0 .. 3
  OPT_NOT_BELOW_0, // max(0, value)
  OPT_AT_LEAST_1,  // the value itself; a value < 1 is refused (MMTTA_ERR_INVALID)
};
static const struct { int key; int* var; OptKind kind; } OPTIONS[] = {
    {MMTTA_OPT_PROFILE_MAIN_KERNEL_ONLY, &mmtta::g_profile_main_only, OPT_AS_IS},
    {MMTTA_OPT_SPLITK_BELOW, &mmtta::g_tune[0], OPT_AT_LEAST_1},
    {MMTTA_OPT_SPLITK_TARGET, &mmtta::g_tune[1], OPT_AT_LEAST_1},
    {MMTTA_OPT_WGRAD_WORKGROUPS, &mmtta::g_tune[2], OPT_AT_LEAST_1},
    {MMTTA_OPT_WGRAD_THIN_SLABS, &mmtta::g_tune[3], OPT_AT_LEAST_1},
    {MMTTA_OPT_IGEMM_PIPELINE, &mmtta::g_igemm_pipeline, OPT_FLAG},
    {MMTTA_OPT_EPILOGUE_VEC16, &mmtta::g_epilogue_vec, OPT_FLAG},
    {MMTTA_OPT_IGEMM_LEAN, &mmtta::g_igemm_lean, OPT_FLAG},
    {MMTTA_OPT_WGRAD_VECTOR_STAGING, &mmtta::g_wgrad_vec, OPT_FLAG},
    {MMTTA_OPT_CLASS_FUSED_MIN_WORKGROUPS, &mmtta::g_cls_fused_min, OPT_NOT_BELOW_0},
    {MMTTA_OPT_THIN_MFMA, &mmtta::g_thin_mfma, OPT_0_TO_3},
    {MMTTA_OPT_IGEMM_FRAGMENT_REUSE, &mmtta::g_igemm_reuse, OPT_FLAG},
    {MMTTA_OPT_LAME_TILED, &mmtta::g_lame_tiled, OPT_FLAG},
    {MMTTA_OPT_RAW_STAGING, &mmtta::g_raw_staging, OPT_BITS01},
    {MMTTA_OPT_HEAD_LOSS_PAIR, &mmtta::g_head_loss_pair, OPT_BITS01},
    {MMTTA_OPT_THIN_LEAN, &mmtta::g_thin_lean, OPT_BITS01},
    {MMTTA_OPT_WGRAD_EPILOGUE_UPDATE, &mmtta::g_wgrad_epilogue_update, OPT_FLAG},
    {MMTTA_OPT_CLS8_PIPELINE, &mmtta::g_cls8_pipeline, OPT_FLAG},
    {MMTTA_OPT_CLS8_LEAN_EPILOGUE, &mmtta::g_cls8_lean_epilogue, OPT_BIT0},      // (bit 1 is reserved: no kernel reads it)
};

extern "C" int mmtta_set_option(int key, int value) {
  for (const auto& o : OPTIONS) {
    if (o.key != key) continue;
    if (o.kind == OPT_AT_LEAST_1 && value < 1) return MMTTA_ERR_INVALID;
    const int prev = *o.var;
    switch (o.kind) {
      case OPT_FLAG: *o.var = value ? 1 : 0; break;
      case OPT_BIT0: *o.var = value & 1; break;
      case OPT_BITS01: *o.var = value & 3; break;
      case OPT_0_TO_3: *o.var = value < 0 ? 0 : (value > 3 ? 3 : value); break;
      case OPT_NOT_BELOW_0: *o.var = value < 0 ? 0 : value; break;
      default: *o.var = value; break;
    }
    return prev;
  }
  return MMTTA_ERR_INVALID;
}

extern "C" const char* mmtta_last_error(void) { return mmtta::g_err; }
extern "C" int mmtta_abi_version(void) { return MMTTA_ABI_VERSION; }
