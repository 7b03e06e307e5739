// nufft_frac_test.cpp -- czt_frac (csrc/czt.hpp) and nufft_turns (csrc/nufft.hpp), the two functions host and device code share
// since the device sorts points too (csrc/nufft_sort.hip), compiled with plain g++ for tests/test_nufft_frac_cpu.py
#include "nufft.hpp"

extern "C" {

void frac_t_frac(double v, int down, unsigned long long *hi, unsigned long long *lo) {
    const phast::CztFrac f = phast::czt_frac(v, down);
    *hi = f.hi;
    *lo = f.lo;
}
double frac_t_turns(double v) { return phast::nufft_turns(phast::czt_frac(v, 0)); }
double frac_t_turns_of(unsigned long long hi, unsigned long long lo) { return phast::nufft_turns(phast::CztFrac{hi, lo}); }

}  // extern "C"
