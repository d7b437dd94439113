// The A/B switches of the launchers (ND_ATTN_*, ND_DKDV_BQ, ND_WGRAD_VARIANT, ND_WGRAD_PLAN, ND_CE) are parsed
// into plain globals when the library loads; no launcher calls getenv.  These two entry points exist for the
// tests, which have to flip a switch after the library is loaded (tests/_switches.py); nothing in the product
// calls them.  Each translation unit keeps its own parse function as the single source of truth: a reload runs
// exactly what the load ran, so outside an ND_ABLATION build it drops the wrong-result values the same way.
#include "common.h"

namespace nd {
void attn_env_reload();
int attn_env_describe(char* buf, int n);
void wgrad_env_reload();
int wgrad_env_describe(char* buf, int n);
void ce_env_reload();
int ce_env_describe(char* buf, int n);
}  // namespace nd

// Parse the environment again and replace the cached switches.  Not thread-safe against concurrent launches.
ND_API int nd_env_reload() {
  nd::attn_env_reload();
  nd::wgrad_env_reload();
  nd::ce_env_reload();
  return 0;
}

// The parsed state as "NAME=value NAME=value ..." (one token per switch, in the switch's own spelling).  Returns
// the length the full text needs (as snprintf); the text is cut to n - 1 characters and always terminated.
ND_API int nd_env_describe(char* buf, int n) {
  if (!buf || n <= 0) return -1;
  int len = 0;
  int (*const parts[])(char*, int) = {nd::attn_env_describe, nd::wgrad_env_describe, nd::ce_env_describe};
  for (auto part : parts) {
    if (len > 0) {
      if (len < n - 1) buf[len] = ' ';
      ++len;
    }
    const int room = len < n ? n - len : 0;
    char none = 0;
    len += part(room ? buf + len : &none, room);
  }
  buf[len < n ? len : n - 1] = 0;
  return len;
}
