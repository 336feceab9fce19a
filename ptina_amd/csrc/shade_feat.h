/* shade_feat.h -- what a scene asks of the SHADE stage, as a bit mask the host decides and the kernels are compiled for.
 *
 * The production SHADE (render_kernel.hip shade_core) carries code for textured materials, the clearcoat and the
 * transmission lobe, an environment map and a list of lights.  A scene that uses none of them pays for the compares,
 * ballots and branches in front of every such region and for their registers.  These are properties of the scene --
 * fixed from one upload of the materials, the lights and the world to the next -- so the host works them out and the
 * launch picks a kernel compiled without the regions (FEAT = MPT_FEAT_PLAIN) or with all of them (MPT_FEAT_GENERIC).
 *
 * Plain C, no dependencies: the host runtime includes it, the kernels take the constants, and a CPU test compiles
 * the two functions on their own.
 */
#pragma once

#include <stdint.h>

enum {
    MPT_FEAT_TEXTURED_MATS = 1,     /* a material the model uses has a texture on any parameter */
    MPT_FEAT_CLEARCOAT = 2,         /* ... has clearcoat non-zero (or textured) */
    MPT_FEAT_TRANSMISSION = 4,      /* ... has transmission non-zero (or textured) */
    MPT_FEAT_WORLD_TEXTURE = 8,     /* the world light has an environment map */
    MPT_FEAT_MANY_LIGHTS = 16,      /* the light list does not hold exactly one light */
    MPT_FEAT_PLAIN = 0,
    MPT_FEAT_GENERIC = 31
    /* The plain kernel is compiled without all five regions and renders the generic kernel's film bit for bit.  That is not free:
     * -ffp-contract=fast fuses the multiply-adds AROUND a removed branch as it pleases, and without the clearcoat and transmission
     * regions a few film elements moved by one ulp (MI355X, s978 128 x 128 x 16: 181 of 16384 without the clearcoat code, 5 without
     * the transmission code) until the two places where the fusing differed were written out -- pt_device.h GTR2 and smithGGX_eval;
     * profiles/r08_ab_experiments.json lists them and how they were found.  A new region compiled out wants the same check.
     * Compiled on its own (unit_eval.hip, kinds MPT_UNIT_DISNEY_*_PLAIN / _LEAN) disney_brdf showed two more: the dot products of its
     * cosines and the two two-product sums of its diffuse lobe (pt_device.h dot_yxz / dot_xyz, "seam 5"), written out the way the
     * render kernels formed them all along; tests/test_reference_disney_cube_gpu.py holds the instantiations word for word. */
};

/* One material as mpt_load_materials receives it: fac[12][4] (parameter k's factor in fac[k*4], basecolor in
 * fac[0..2]; order of mtllib.py:44-56, clearcoat = 8, transmission = 10), tex[12] texture ids (-1: none) or null.
 * A parameter counts as used when its factor is non-zero (a NaN is) or it has a texture: "zero but textured" is used. */
static inline int shade_feat_material(const float *fac, const int32_t *tex) {
    int bits = 0;
    if (tex)
        for (int k = 0; k < 12; k++)
            if (tex[k] != -1) bits |= MPT_FEAT_TEXTURED_MATS;
    if (fac[8 * 4] != 0.0f || (tex && tex[8] != -1)) bits |= MPT_FEAT_CLEARCOAT;
    if (fac[10 * 4] != 0.0f || (tex && tex[10] != -1)) bits |= MPT_FEAT_TRANSMISSION;
    return bits;
}

/* The scene's mask: the bits of every material the model uses (records 0 .. max_mtlid; records that were never
 * loaded are all-zero and add nothing), of the default material (always: faces with material id -1 take it), and
 * what the light list and the world light add. */
static inline int shade_feat_scene(const unsigned char *mat_bits, int nmats, int max_mtlid, int default_bits,
                                   int nlights, int world_tex) {
    int bits = default_bits;
    for (int i = 0; i < nmats && i <= max_mtlid; i++) bits |= mat_bits[i];
    if (world_tex != -1) bits |= MPT_FEAT_WORLD_TEXTURE;
    if (nlights != 1) bits |= MPT_FEAT_MANY_LIGHTS;
    return bits;
}

/* Two instantiations are built: a scene with any bit set takes the generic one. */
static inline int shade_feat_instantiation(int scene_bits, int shade_spec) {
    return (shade_spec && scene_bits == MPT_FEAT_PLAIN) ? MPT_FEAT_PLAIN : MPT_FEAT_GENERIC;
}

/* The lean variant of the plain instantiation: SHADE without the subsurface and sheen terms of the diffuse lobe (pt_device.h
 * disney_brdf / disney_bounce, LEAN).  It is no bit of the mask above -- a scene with sheen or subsurface stays MPT_FEAT_PLAIN and
 * takes the plain kernel as before -- but a second, independent answer the launch asks for when the instantiation is plain.
 *
 * A material is lean when sheen (parameter 6) and subsurface (parameter 5) are exactly zero and untextured: the dropped terms are
 * ss * 0 and sheencolor * (Foh * 0), so -0.0 counts as zero, and any other value, a NaN included, does not. */
static inline int shade_lean_material(const float *fac, const int32_t *tex) {
    if (tex && (tex[5] != -1 || tex[6] != -1)) return 0;
    return fac[5 * 4] == 0.0f && fac[6 * 4] == 0.0f;
}

/* The scene's answer: every material the model uses (records 0 .. max_mtlid; records that were never loaded are all-zero, which
 * is lean) and the default material (always) are lean.  mat_lean[i]: shade_lean_material of record i. */
static inline int shade_lean_scene(const unsigned char *mat_lean, int nmats, int max_mtlid, int default_lean) {
    if (!default_lean) return 0;
    for (int i = 0; i < nmats && i <= max_mtlid; i++)
        if (!mat_lean[i]) return 0;
    return 1;
}

/* Three instantiations are built: generic, plain, and plain + lean.  inst: what shade_feat_instantiation chose; lean_on: 0 keeps
 * every plain scene on the plain kernel (A/B timing). */
static inline int shade_lean_instantiation(int inst, int scene_lean, int lean_on) {
    return inst == MPT_FEAT_PLAIN && scene_lean && lean_on;
}
