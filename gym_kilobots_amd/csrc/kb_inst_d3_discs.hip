// kernel instantiations for drive law KB_DRIVE_SIMPLE_PHOTOTAXIS in scenes whose objects are all discs (POLY = false)
#include "kb_step_kernel.h"

namespace kb {
static constexpr bool in_unit(const Variant &v) { return v.drive == KB_DRIVE_SIMPLE_PHOTOTAXIS && !v.poly; }
static const bool registered = register_unit<in_unit>();
}  // namespace kb
