// The one reader of the LAMP_* environment switches (table and parsing rules: switches.h).
#include "switches.h"
#include <algorithm>
#include <cstdlib>

namespace lamp {
namespace {
enum SwKind { BOOL, INT, LETTER };
int64_t read_switch(const char* name, SwKind kind, int64_t dflt, int64_t lo) {
  const char* e = getenv(name);
  switch (kind) {
    case BOOL: return dflt ? !(e && e[0] == '0') : (e && e[0] == '1');
    case INT: return e ? std::max<int64_t>(lo, atoll(e)) : dflt;
    case LETTER: return e ? e[0] : 0;
  }
  return dflt;
}
}  // namespace

#define LAMP_SWITCH_READ(member, name, kind, dflt, lo, doc) s.member = (SwType_##kind)read_switch(name, kind, dflt, lo);
const Switches& sw() {
  static const Switches once = [] { Switches s; LAMP_SWITCHES_ONCE(LAMP_SWITCH_READ) return s; }();
  return once;
}
SwitchesNow sw_now() {
  SwitchesNow s;
  LAMP_SWITCHES_PER_CALL(LAMP_SWITCH_READ)
  return s;
}
#undef LAMP_SWITCH_READ

}  // namespace lamp
