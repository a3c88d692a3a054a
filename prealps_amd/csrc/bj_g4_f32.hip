// bj_g4.hip compiled for fp32 records (PREALPS_BJ_BAND_PRECISION=single), blocks of up to 192 rows; see there.
#define G4_F32 1
#include "bj_g4.hip"
