// ABI bookkeeping: version, per-thread error text and the table of tuning hooks.
#include <cstring>
#include <string>

#include "common.h"

namespace lea {
namespace {
thread_local char g_err[512] = {0};
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

void clear_error() { g_err[0] = 0; }

// zero-initialised before any unit's registrars run
namespace {
constexpr int kMaxHooks = 64;
TuningHook g_hooks[kMaxHooks];
int g_nhooks = 0;
}  // namespace

TuningRegistrar::TuningRegistrar(const char* setter, int nargs, void (*get)(int*)) {
  if (g_nhooks < kMaxHooks) g_hooks[g_nhooks++] = TuningHook{setter, nargs, get};
}

}  // namespace lea

extern "C" int lea_abi_version(void) { return LEA_ABI_VERSION; }

extern "C" const char* lea_last_error(void) { return lea::g_err; }

extern "C" const char* lea_tuning_name(int i) {
  return i >= 0 && i < lea::g_nhooks ? lea::g_hooks[i].setter : nullptr;
}

extern "C" int lea_tuning_get(const char* setter, int* values, int capacity) {
  lea::clear_error();
  for (int i = 0; setter && i < lea::g_nhooks; ++i) {
    const lea::TuningHook& h = lea::g_hooks[i];
    if (strcmp(h.setter, setter) != 0) continue;
    if (!values || capacity < h.nargs) {
      lea::set_error("lea_tuning_get: %s has %d values, capacity %d", setter, h.nargs, values ? capacity : 0);
      return -1;
    }
    h.get(values);
    return h.nargs;
  }
  lea::set_error("lea_tuning_get: unknown setter %s", setter ? setter : "(null)");
  return -1;
}
