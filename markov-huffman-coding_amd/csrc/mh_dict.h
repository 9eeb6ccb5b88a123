// mh_dict.h — the dictionary of the dictionary search (include/mh.h, "DICTIONARY SEARCH IN BATCHES"): an Aho-Corasick
// automaton turned into a full DFA, built on the host (mh_dict_host.cpp, no HIP in it), and its device image as the kernels
// of mh_find.hip read it.  No HIP in this header either: the fuzz program (sanitize/fuzz_dict.cpp) builds with the host
// source alone.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mhd {

// The device image, one allocation: cls u8[256] | trans u16[states x ncls] | out_off u32[states + 1] | out_pat u32[n_out] |
// depth u8[states] | out_len u8[n_out], every part 16-byte aligned.  Rows 0 .. R-1 of trans are what the kernels keep in LDS.
struct DictDev {
    const uint8_t *cls;             // byte -> class; class 0: the bytes of no pattern
    const uint16_t *trans;          // row s, column cls: target state | 0x8000 when the target has outputs
    const uint32_t *out_off;        // CSR over the states
    const uint32_t *out_pat;        // ascending pattern numbers within a state
    const uint8_t *depth;           // the longest pattern prefix a state stands for
    const uint8_t *out_len;         // the patterns' lengths, beside out_pat
    uint32_t ncls, states, max_len;
};

struct DictImage {
    size_t off_trans, off_out_off, off_out_pat, off_depth, off_out_len, total;
};
inline DictImage dict_image(size_t states, size_t ncls, size_t n_out) {
    auto up = [](size_t v) { return (v + 15) & ~size_t(15); };
    DictImage l;
    l.off_trans = 256;
    l.off_out_off = up(l.off_trans + states * ncls * 2);
    l.off_out_pat = up(l.off_out_off + (states + 1) * 4);
    l.off_depth = up(l.off_out_pat + n_out * 4);
    l.off_out_len = up(l.off_depth + states);
    l.total = up(l.off_out_len + n_out);
    return l;
}

}  // namespace mhd

struct mh_dict {
    uint8_t cls[256];
    std::vector<uint16_t> trans;
    std::vector<uint32_t> out_off, out_pat;
    std::vector<uint8_t> depth, out_len;
    uint32_t n = 0, max_len = 0, flags = 0, ncls = 0, states = 0;
    // the device image (mh_api_find.cpp uploads and frees it; null without a device)
    void *d_image = nullptr;
    int device = -1;
    mhd::DictDev dev{};
};

namespace mhd {

// What mh_dict_create and mh_dict_free call when the library's device side is linked in (mh_api_find.cpp sets them while the
// library loads); null in a host-only program.  upload returns an MH_* code; MH_OK with d_image null: no usable device.
extern int (*g_upload)(mh_dict *d);
extern void (*g_release)(mh_dict *d);

}  // namespace mhd
