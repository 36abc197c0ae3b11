// Library-wide host state and checks: the per-thread error text behind iclr17_last_error, the
// launch check, the shape checks of the entry points, and the deconv tap enumeration the packing
// code shares with the engine's tap table (declared in common.h).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

namespace iclr17 {

namespace {
thread_local char g_err[512];
}  // namespace

void set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  int n = snprintf(g_err, sizeof(g_err), "iclr17 error %d: ", code);
  if (n < 0) n = 0;
  vsnprintf(g_err + n, sizeof(g_err) - n, fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(ICLR17_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ICLR17_ELAUNCH;
  }
  return ICLR17_OK;
}

int check_image(int B, int H, int W, int N) {
  ICLR17_REQUIRE(B > 0 && H > 0 && W > 0, ICLR17_EINVAL, "bad shape B=%d H=%d W=%d", B, H, W);
  ICLR17_REQUIRE(H % 16 == 0 && W % 16 == 0, ICLR17_EINVAL,
                 "image height/width must be multiples of 16 (got %dx%d)", H, W);
  ICLR17_REQUIRE(N == 128 || N == 192, ICLR17_EUNSUPPORTED, "channel count N=%d unsupported (128, 192)", N);
  return ICLR17_OK;
}

int check_grid(const char* what, int B, int h, int w, int N) {
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0, ICLR17_EINVAL, "%s: bad shape", what);
  ICLR17_REQUIRE(N == 128 || N == 192, ICLR17_EUNSUPPORTED, "channel count N=%d unsupported", N);
  return ICLR17_OK;
}

void deconv_phase_taps(int K, int s, int p, int ry, int rx, int* kh_out, int* kw_out, int* count) {
  *count = for_each_deconv_tap(K, s, p, ry, rx, [&, n = 0](int, int, int kh, int kw) mutable {
    kh_out[n] = kh;
    kw_out[n] = kw;
    ++n;
  });
}

}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_version(void) { return 1; }

int iclr17_last_error(char* buf, size_t len) {
  const size_t n = strlen(g_err);
  if (buf != nullptr && len > 0) {
    const size_t c = n < len - 1 ? n : len - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return (int)n;
}

}  // extern "C"
