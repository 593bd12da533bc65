// dirt_shade_albedo.hip -- the second translation unit of dirt_shade.hip: its kernels with ALBEDO = true (a pixel's colour read
// from a separate image, its gradient written to one) and the entry points dirt_shade_albedo_forward / _backward.  The source
// is one; it is compiled twice so that the 29 kernels of the channel path and these 37 build side by side.
#define DIRT_SHADE_ALBEDO_UNIT 1
#include "dirt_shade.hip"
