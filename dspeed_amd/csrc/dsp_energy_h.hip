// dsp_energy_h.hip -- the register-resident energy kernel built for the 4-point pick-off mode h: the second translation unit of
// dsp_energy.hip (see "This file is two translation units" there), compiled beside the first so that the library's build takes no longer.
#define DSP_ENERGY_UNIT 1
#include "dsp_energy.hip"
