/*
 * oslam_colour_lerp.h -- the blend of eight colour words at a point, shared by the read of a volume's colour buffer
 * (oslam_colour.hip) and the read of the whole map's colours (oslam_world_colour.hip), so that both round alike
 * (include/oslam.h at oslam_volume_colours).  Device code.
 */
#ifndef OSLAM_COLOUR_LERP_H
#define OSLAM_COLOUR_LERP_H

#include <math.h>
#include <stdint.h>

__device__ __forceinline__ float colour_lerp(float a, float b, float f) { return a * (1.0f - f) + b * f; }

/* one channel (bits sh .. sh + 7) of the eight corners, trilinear with the ray cast's order, rounded and clipped */
__device__ __forceinline__ uint32_t colour_channel(const uint32_t c[8], int sh, float fx, float fy, float fz)
{
    const float c00 = colour_lerp((float)((c[0] >> sh) & 0xffu), (float)((c[1] >> sh) & 0xffu), fx);
    const float c10 = colour_lerp((float)((c[2] >> sh) & 0xffu), (float)((c[3] >> sh) & 0xffu), fx);
    const float c01 = colour_lerp((float)((c[4] >> sh) & 0xffu), (float)((c[5] >> sh) & 0xffu), fx);
    const float c11 = colour_lerp((float)((c[6] >> sh) & 0xffu), (float)((c[7] >> sh) & 0xffu), fx);
    const float val = floorf(colour_lerp(colour_lerp(c00, c10, fy), colour_lerp(c01, c11, fy), fz) + 0.5f);
    return (uint32_t)fminf(fmaxf(val, 0.0f), 255.0f);
}

#endif /* OSLAM_COLOUR_LERP_H */
