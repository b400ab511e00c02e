// Host build of svt-av1_amd/csrc/fmt_dispatch.h for tests/test_fmt_dispatch_host.py: one line per (family, pix_bytes, bd) with the tag the lambda received,
//     <family> <pix_bytes> <bd> <bytes of the tag's sample type> <the tag's bit depth>
#include <stdio.h>
#include "../svt-av1_amd/csrc/fmt_dispatch.h"

int main() {
    const int depths[] = {8, 9, 10, 11, 12, 16};
    for (int pix_bytes = 1; pix_bytes <= 2; pix_bytes++)
        for (int bd : depths) {
            const auto report = [&](const char* family) {
                return [=](auto f) { printf("%s %d %d %d %d\n", family, pix_bytes, bd, (int)sizeof(typename decltype(f)::pix), (int)decltype(f)::bd); };
            };
            svt_for_pix(pix_bytes, report("pix"));
            svt_for_fmt(pix_bytes, bd, report("fmt"));
            svt_for_fmt12(pix_bytes, bd, report("fmt12"));
        }
    return 0;
}
