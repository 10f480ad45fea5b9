// per-thread error text, ABI version, options / context
#include <stdarg.h>

#include "pp_common.h"

static thread_local char g_err[512] = "";

void pp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* pp_last_error(void) { return g_err; }
extern "C" int pp_abi_version(void) { return PP_ABI_VERSION; }

// ------------------------------------------------------------------------------------------------ options / context
struct PPOptionDef { const char* name; int dflt, lo, hi; };
static const PPOptionDef g_opt_def[PP_OPT_COUNT] = {
    {"mlp_fused", 1, 0, 1},          {"grid_chunks", 0, 0, 4096},  {"nerf_split", 1, 0, 1},
    {"mlp_split", 31, 0, 31},        {"mlp_wgs", 0, 0, 4096},      {"nerf_chain", 3, 0, 3},
    {"mlp_pack", 1, 0, 1},           {"warp_lean", 1, 0, 1},
};
// compiled-in defaults: constants, never written after static initialisation
static const struct PPDefaults {
  int v[PP_OPT_COUNT];
  PPDefaults() { for (int i = 0; i < PP_OPT_COUNT; ++i) v[i] = g_opt_def[i].dflt; }
} g_defaults;

const int* pp_options(const void* ctx) { return ctx ? static_cast<const PPContext*>(ctx)->opt : g_defaults.v; }

int pp_num_cus() {
  static const int n = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        cus > 0)
      return cus;
    return 256;
  }();
  return n;
}

static int opt_find(const char* name) {
  for (int i = 0; i < PP_OPT_COUNT; ++i) if (name && strcmp(name, g_opt_def[i].name) == 0) return i;
  return -1;
}

extern "C" int pp_context_create(void** ctx) {
  PP_REQUIRE(ctx, "null pointer");
  PPContext* c = new PPContext;
  for (int i = 0; i < PP_OPT_COUNT; ++i) c->opt[i] = g_opt_def[i].dflt;
  c->pack = nullptr;
  c->pack_params[0] = c->pack_params[1] = nullptr;
  c->lean_acts = c->lean_scratch = c->lean_params = nullptr;
  c->ord = nullptr;
  c->ord_wgs = c->ord_cap = c->ord_rays = 0;
  c->nerf_ord = nullptr;
  c->join_open = c->join_pending = false;
  *ctx = c;
  return PP_OK;
}

extern "C" int pp_context_destroy(void* ctx) {
  if (!ctx) return PP_OK;
  delete static_cast<PPContext*>(ctx);
  return PP_OK;
}

extern "C" int pp_context_set_option(void* ctx, const char* name, int32_t value) {
  PP_REQUIRE(ctx, "null context (the compiled-in defaults cannot be changed: create a context)");
  const int i = opt_find(name);
  if (i < 0) { pp_set_error("pp_context_set_option: unknown option '%s'", name ? name : "(null)"); return PP_ERR_INVALID_ARG; }
  if (value < g_opt_def[i].lo || value > g_opt_def[i].hi) {
    pp_set_error("pp_context_set_option: %s = %d outside [%d, %d]", name, value, g_opt_def[i].lo, g_opt_def[i].hi);
    return PP_ERR_INVALID_ARG;
  }
  if (i == PP_OPT_NERF_CHAIN && value != 0 && value != 3) {
    pp_set_error("pp_context_set_option: nerf_chain = %d selected a hybrid of the fused and the layer-by-layer route, which is retired: "
                 "3 (fused) or 0 (layer by layer)", value);
    return PP_ERR_INVALID_ARG;
  }
  static_cast<PPContext*>(ctx)->opt[i] = value;
  return PP_OK;
}

extern "C" int pp_context_get_option(const void* ctx, const char* name, int32_t* value) {
  const int i = opt_find(name);
  if (i < 0 || !value) { pp_set_error("pp_context_get_option: unknown option '%s'", name ? name : "(null)"); return PP_ERR_INVALID_ARG; }
  *value = ctx ? static_cast<const PPContext*>(ctx)->opt[i] : g_opt_def[i].dflt;
  return PP_OK;
}
