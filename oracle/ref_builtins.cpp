// The two transcendental built-ins of oracle/glsl_shim.h, in a translation unit of their own:
// vcrt_math.h's double constants must not be compiled with -fsingle-precision-constant, which
// the shader's translation unit needs. TEST INFRASTRUCTURE ONLY.
#include <cmath>

#include "../vulkancomputeraytracing_amd/csrc/vcrt_math.h"

extern "C" float ref_builtin_sin(float x) { return vcrt::sin_canonical(x); }

// tan widens to double, one rounding to fp32 (as make_camera's tan_fn is used)
extern "C" float ref_builtin_tan(float x) { return (float)std::tan((double)x); }
