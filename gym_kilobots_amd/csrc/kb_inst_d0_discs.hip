// kernel instantiations for drive law KB_DRIVE_VELOCITY in scenes whose objects are all discs (BASELINE config 4):
// the kilobot - polygon contact code and its per-slot registers fold away (POLY = false)
#include "kb_step_kernel.h"

namespace kb {
static constexpr bool in_unit(const Variant &v) { return v.drive == KB_DRIVE_VELOCITY && !v.poly; }
static const bool registered = register_unit<in_unit>();
}  // namespace kb
