// bj_g4.hip compiled for the PAIR launch (two blocks of one class per wavefront), blocks of up to 192 rows; see there.
#define G4_PAIR 1
#include "bj_g4.hip"
