// glgym_rng.h -- internal interface between the C ABI (glgym.hip) and the NumPy-stream kernels (glgym_rng.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// glgym_rng_crop_noise: one lane per environment on `stream`, no host copy, allocation or synchronisation (capturable).
// crop_p: T [34][ld] or nullptr (the streams only advance by 34 draws); p0: the handle's float32 p[128..161] on the device;
// rng_state: uint64 [5][ld].  T = float | double (instantiated in glgym_rng.hip).
template <class T>
hipError_t rng_crop_noise_launch(T* crop_p, int B, int ld, const float* p0, double scale, uint64_t* rng_state, hipStream_t stream);

// glgym_rng_reset_draw: start (year, day) of every masked environment (mask == nullptr: all) from its stream.
hipError_t rng_reset_draw_launch(int B, int ld, const unsigned char* mask, uint64_t* rng_state, int n_years, int n_days,
                                 const int* start_rows, const float* start_days, int* w_off, float* start_day, hipStream_t stream);
