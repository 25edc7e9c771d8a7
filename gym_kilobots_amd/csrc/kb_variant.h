// kb_variant.h -- which instantiation of kb_step_kernel runs a handle: the variant key, the one list of the instantiations
// the library carries, and the rule that picks one.  Plain C++17 without HIP (tests/test_variant_cpu.py compiles it with
// the system compiler).
#pragma once
#include <initializer_list>

#include "kilobots_hip.h"

namespace kb {

constexpr int KB_LIGHT_GENERAL = 99;   // kernel template value: any light model other than NONE / single CIRCULAR

// the template arguments of one kb_step_kernel instantiation, in template order (kb_step_kernel.h says what each one does)
struct Variant {
    int drive, light;
    bool obj;
    int fn, tier;
    bool poly, sense, sleep;
};
constexpr bool operator==(const Variant &a, const Variant &b) {
    return a.drive == b.drive && a.light == b.light && a.obj == b.obj && a.fn == b.fn && a.tier == b.tier && a.poly == b.poly &&
           a.sense == b.sense && a.sleep == b.sleep;
}

constexpr int LIGHT_CLASSES[] = {KB_LIGHT_NONE, KB_LIGHT_CIRCULAR, KB_LIGHT_GENERAL};
constexpr int NUM_VARIANTS = 176;
struct VariantList { Variant v[NUM_VARIANTS]; int n; };

// every instantiation of the library; each kb_inst_*.hip unit compiles a slice of it
constexpr VariantList make_variants() {
    VariantList l{};
    for (int d : {KB_DRIVE_VELOCITY, KB_DRIVE_ACCEL, KB_DRIVE_MOTORS, KB_DRIVE_SIMPLE_PHOTOTAXIS, KB_DRIVE_PHOTOTAXIS})
        for (int L : LIGHT_CLASSES) {
            if (L == KB_LIGHT_NONE && (d == KB_DRIVE_SIMPLE_PHOTOTAXIS || d == KB_DRIVE_PHOTOTAXIS)) continue;   // (kb_create: phototaxis needs a light)
            for (bool sleep : {false, true}) {
                for (int tier : {0, 2}) l.v[l.n++] = {d, L, false, 0, tier, true, true, sleep};       // no objects: 128 / 80 VGPRs
                for (bool poly : {true, false})                                                       // objects (all discs: POLY = false)
                    for (int tier : {0, 1}) l.v[l.n++] = {d, L, true, 0, tier, poly, true, sleep};    // ... 128 VGPRs / one-wave workgroup at 256
            }
        }
    // num_bots == 1024 with the full workgroup: compile-time LDS layout (no light; the ones with objects carry no sleep state)
    for (bool sense : {false, true}) {
        for (bool sleep : {false, true}) l.v[l.n++] = {KB_DRIVE_VELOCITY, KB_LIGHT_NONE, false, 1024, 0, true, sense, sleep};
        for (bool poly : {true, false}) l.v[l.n++] = {KB_DRIVE_VELOCITY, KB_LIGHT_NONE, true, 1024, 0, poly, sense, false};
    }
    // mixed drive laws: one-wave workgroups (tier 1) or the full workgroup (tier 3), 256 VGPRs either way
    for (int L : LIGHT_CLASSES)
        for (int tier : {1, 3})
            for (bool sleep : {false, true}) l.v[l.n++] = {KB_DRIVE_MIXED, L, true, 0, tier, true, true, sleep};
    return l;
}
inline constexpr VariantList kb_variants = make_variants();
static_assert(kb_variants.n == NUM_VARIANTS, "NUM_VARIANTS is the length of the list");

// position of a key in kb_variants, -1 if the library has no such instantiation
constexpr int variant_index(const Variant &v) {
    for (int i = 0; i < NUM_VARIANTS; ++i)
        if (kb_variants.v[i] == v) return i;
    return -1;
}

// what of a handle decides its instantiation
struct Shape {
    int drive_mode, light_type;     // kb_config
    bool objects, all_discs;        // num_objects > 0; ... and every fixture is a circle
    bool sense, sleep;              // sense_radius > 0; allow_sleep
    int threads, tier;              // workgroup size; register budget of the kernels without objects (kb_launch.h: compact_tier)
    bool fixed_1024;                // kb_launch.h: fixed_1024
};

constexpr Variant select_variant(const Shape &s) {
    // GradientLight, MomentumLight, CompositeLight: one general kernel
    const int L = (s.light_type == KB_LIGHT_NONE || s.light_type == KB_LIGHT_CIRCULAR) ? s.light_type : KB_LIGHT_GENERAL;
    const bool poly = !(s.objects && s.all_discs);      // all discs: without the kilobot - polygon contact code
    if (s.fixed_1024) return {KB_DRIVE_VELOCITY, KB_LIGHT_NONE, s.objects, 1024, 0, poly, s.sense, s.sleep};
    if (s.drive_mode == KB_DRIVE_MIXED) return {KB_DRIVE_MIXED, L, true, 0, s.threads == 64 ? 1 : 3, true, true, s.sleep};
    // with objects a one-wave workgroup runs the 256-VGPR instantiation; without, compact_tier decides between 128 and 80 VGPRs
    return {s.drive_mode, L, s.objects, 0, s.objects ? (s.threads <= 64 ? 1 : 0) : s.tier, poly, true, s.sleep};
}

}  // namespace kb
