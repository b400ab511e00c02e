// fmt_dispatch.h — which kernel instance a launcher runs for a sample format, chosen in one place.  Plain C++17, nothing from HIP: tests/fmt_dispatch_host.cpp
// pins the three rules below on the host.
//
// A launcher states its kernel and its argument list once, inside a generic lambda that receives the tag of the chosen format:
//
//     svt_for_fmt(pix_bytes, bd, [&](auto f) {
//         using PIX = typename decltype(f)::pix;
//         hipLaunchKernelGGL((some_kernel<PIX, decltype(f)::bd>), grid, block, 0, st, (const PIX*)src, stride, (PIX*)dst, ...);
//     });
//
// The lambda's result, if it has one, is returned.  Values the C-ABI layer refuses before they arrive still select what they always selected.
#pragma once
#include <stdint.h>

template <class P, int B> struct SvtFmt { using pix = P; static constexpr int bd = B; };   // bd 0: the bit depth is no template argument of the kernel

// u8 | u16
template <class F> auto svt_for_pix(int pix_bytes, F&& f) {
    if (pix_bytes == 1) return f(SvtFmt<uint8_t, 0>{});
    return f(SvtFmt<uint16_t, 0>{});
}
// (u8, 8) | (u16, 8) | (u16, 10)
template <class F> auto svt_for_fmt(int pix_bytes, int bd, F&& f) {
    if (pix_bytes == 1) return f(SvtFmt<uint8_t, 8>{});
    if (bd == 8) return f(SvtFmt<uint16_t, 8>{});
    return f(SvtFmt<uint16_t, 10>{});
}
// (u8, 8) | (u16, 8) | (u16, 10) | (u16, 12)
template <class F> auto svt_for_fmt12(int pix_bytes, int bd, F&& f) {
    if (pix_bytes == 1) return f(SvtFmt<uint8_t, 8>{});
    if (bd == 8) return f(SvtFmt<uint16_t, 8>{});
    if (bd == 10) return f(SvtFmt<uint16_t, 10>{});
    return f(SvtFmt<uint16_t, 12>{});
}
