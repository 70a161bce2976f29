/*
 * oslam_ply.c -- PLY point clouds with normals, in C: what the reference gets from
 * pcl::io::loadPLYFile<pcl::PointNormal> (pcl/alignment/src/alignment.cpp:212,241) and writes
 * with pcl::PLYWriter (pcl/voxel_grid/voxel_grid.cpp:27-29) or matlab/write_ply_cloud.m.
 * Host-only.  Reads `format ascii 1.0` and `format binary_little_endian 1.0`; the vertex
 * element must come first; it needs x, y, z and normals named nx ny nz or
 * normal_x normal_y normal_z (any scalar type, any other properties are skipped).  Elements after the
 * vertices (the faces that oslam_ply_write_mesh writes) are skipped.
 */
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oslam.h"

static int type_size(const char *t)
{
    if (!strcmp(t, "char") || !strcmp(t, "uchar") || !strcmp(t, "int8") || !strcmp(t, "uint8")) return 1;
    if (!strcmp(t, "short") || !strcmp(t, "ushort") || !strcmp(t, "int16") || !strcmp(t, "uint16")) return 2;
    if (!strcmp(t, "int") || !strcmp(t, "uint") || !strcmp(t, "float") || !strcmp(t, "int32") ||
        !strcmp(t, "uint32") || !strcmp(t, "float32")) return 4;
    if (!strcmp(t, "double") || !strcmp(t, "float64")) return 8;
    return 0;
}

static double read_scalar(const unsigned char *p, const char *t)
{
    if (!strcmp(t, "float") || !strcmp(t, "float32")) { float v; memcpy(&v, p, 4); return v; }
    if (!strcmp(t, "double") || !strcmp(t, "float64")) { double v; memcpy(&v, p, 8); return v; }
    if (!strcmp(t, "char") || !strcmp(t, "int8")) return (signed char)p[0];
    if (!strcmp(t, "uchar") || !strcmp(t, "uint8")) return p[0];
    if (!strcmp(t, "short") || !strcmp(t, "int16")) { short v; memcpy(&v, p, 2); return v; }
    if (!strcmp(t, "ushort") || !strcmp(t, "uint16")) { unsigned short v; memcpy(&v, p, 2); return v; }
    if (!strcmp(t, "int") || !strcmp(t, "int32")) { int v; memcpy(&v, p, 4); return v; }
    { unsigned v; memcpy(&v, p, 4); return v; }
}

#define MAX_PROPS 64

int oslam_ply_read(const char *path, float **xyz_out, float **nrm_out, size_t *n_out)
{
    FILE *f;
    char line[1024], types[MAX_PROPS][16];
    int nprop = 0, ascii = -1, in_vertex = 0, seen_vertex = 0, off[MAX_PROPS], slot[MAX_PROPS], rec = 0, i;
    int have[6] = {0, 0, 0, 0, 0, 0};
    size_t n = 0, v;
    float *xyz = NULL, *nrm = NULL;
    unsigned char *buf = NULL;
    int rc = OSLAM_E_INVALID;
    if (!path || !xyz_out || !nrm_out || !n_out) return OSLAM_E_INVALID;
    *xyz_out = *nrm_out = NULL;
    *n_out = 0;
    f = fopen(path, "rb");
    if (!f) return OSLAM_E_INVALID;
    if (!fgets(line, sizeof line, f) || strncmp(line, "ply", 3)) goto done;
    while (fgets(line, sizeof line, f)) {
        char a[64] = "", b[64] = "", c[64] = "";
        int k = sscanf(line, "%63s %63s %63s", a, b, c);
        if (k < 1) continue;
        if (!strcmp(a, "end_header")) break;
        if (!strcmp(a, "format")) {
            if (!strcmp(b, "ascii")) ascii = 1;
            else if (!strcmp(b, "binary_little_endian")) ascii = 0;
            else goto done;                                   /* big endian: not supported */
        } else if (!strcmp(a, "element")) {
            in_vertex = !strcmp(b, "vertex");
            if (in_vertex) {
                if (seen_vertex) goto done;
                seen_vertex = 1;
                n = (size_t)strtoull(c, NULL, 10);
            } else if (!seen_vertex) {
                goto done;                                    /* an element before the vertices */
            }
        } else if (!strcmp(a, "property") && in_vertex) {
            static const char *names[6][2] = {{"x", "x"}, {"y", "y"}, {"z", "z"}, {"nx", "normal_x"},
                                              {"ny", "normal_y"}, {"nz", "normal_z"}};
            if (!strcmp(b, "list") || nprop == MAX_PROPS || !type_size(b)) goto done;
            snprintf(types[nprop], sizeof types[nprop], "%.15s", b);
            off[nprop] = rec;
            rec += type_size(b);
            slot[nprop] = -1;
            for (i = 0; i < 6; i++)
                if (!strcmp(c, names[i][0]) || !strcmp(c, names[i][1])) { slot[nprop] = i; have[i] = 1; }
            nprop++;
        }
    }
    if (ascii < 0 || !seen_vertex || !(have[0] && have[1] && have[2] && have[3] && have[4] && have[5])) goto done;
    xyz = (float *)malloc(sizeof(float) * 3 * (n ? n : 1));
    nrm = (float *)malloc(sizeof(float) * 3 * (n ? n : 1));
    if (!xyz || !nrm) { rc = OSLAM_E_NOMEM; goto done; }
    if (ascii) {
        for (v = 0; v < n; v++) {
            for (i = 0; i < nprop; i++) {
                double d;
                if (fscanf(f, "%lf", &d) != 1) goto done;
                if (slot[i] >= 0 && slot[i] < 3) xyz[3 * v + slot[i]] = (float)d;
                else if (slot[i] >= 3) nrm[3 * v + slot[i] - 3] = (float)d;
            }
        }
    } else {
        buf = (unsigned char *)malloc((size_t)rec * (n ? n : 1));
        if (!buf) { rc = OSLAM_E_NOMEM; goto done; }
        if (fread(buf, (size_t)rec, n, f) != n) goto done;
        for (v = 0; v < n; v++)
            for (i = 0; i < nprop; i++) {
                if (slot[i] < 0) continue;
                float d = (float)read_scalar(buf + v * (size_t)rec + off[i], types[i]);
                if (slot[i] < 3) xyz[3 * v + slot[i]] = d; else nrm[3 * v + slot[i] - 3] = d;
            }
    }
    *xyz_out = xyz;
    *nrm_out = nrm;
    *n_out = n;
    xyz = nrm = NULL;
    rc = OSLAM_OK;
done:
    free(xyz);
    free(nrm);
    free(buf);
    fclose(f);
    return rc;
}

/* the header up to the vertex properties (with_rgb: red, green, blue behind the normal), then (n_faces != (size_t)-1) the
 * face element, then end_header */
static void ply_header(FILE *f, int binary, size_t n, size_t n_faces, int with_rgb)
{
    fprintf(f, "ply\nformat %s 1.0\ncomment written by liboslam_hip\nelement vertex %zu\n"
               "property float x\nproperty float y\nproperty float z\n"
               "property float normal_x\nproperty float normal_y\nproperty float normal_z\n",
            binary ? "binary_little_endian" : "ascii", n);
    if (with_rgb) fprintf(f, "property uchar red\nproperty uchar green\nproperty uchar blue\n");
    if (n_faces != (size_t)-1) fprintf(f, "element face %zu\nproperty list uchar int vertex_indices\n", n_faces);
    fprintf(f, "end_header\n");
}

/* rgb NULL: without colour */
static void ply_vertices(FILE *f, int binary, const float *xyz, const float *nrm, const uint8_t *rgb, size_t n)
{
    size_t v;
    for (v = 0; v < n; v++) {
        if (binary) {
            fwrite(xyz + 3 * v, sizeof(float), 3, f);
            fwrite(nrm + 3 * v, sizeof(float), 3, f);
            if (rgb) fwrite(rgb + 3 * v, 1, 3, f);
        } else {
            fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g", xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], nrm[3 * v], nrm[3 * v + 1],
                    nrm[3 * v + 2]);
            if (rgb) fprintf(f, " %u %u %u", (unsigned)rgb[3 * v], (unsigned)rgb[3 * v + 1], (unsigned)rgb[3 * v + 2]);
            fputc('\n', f);
        }
    }
}

/* oslam_ply_write and oslam_ply_write_colour (rgb given) after their checks */
static int write_cloud(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t n, int binary)
{
    FILE *f = fopen(path, "wb");
    if (!f) return OSLAM_E_INVALID;
    ply_header(f, binary, n, (size_t)-1, rgb != NULL);
    ply_vertices(f, binary, xyz, nrm, rgb, n);
    return fclose(f) ? OSLAM_E_INVALID : OSLAM_OK;
}

int oslam_ply_write(const char *path, const float *xyz, const float *nrm, size_t n, int binary)
{
    if (!path || !xyz || !nrm) return OSLAM_E_INVALID;
    return write_cloud(path, xyz, nrm, NULL, n, binary);
}

int oslam_ply_write_colour(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t n, int binary)
{
    if (!path || !xyz || !nrm || !rgb) return OSLAM_E_INVALID;
    return write_cloud(path, xyz, nrm, rgb, n, binary);
}

static int write_mesh(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t nv, const uint32_t *tri,
                      size_t nt, int binary);

int oslam_ply_write_mesh(const char *path, const float *xyz, const float *nrm, size_t nv, const uint32_t *tri, size_t nt, int binary)
{
    if (!path || (nv && (!xyz || !nrm)) || (nt && !tri)) return OSLAM_E_INVALID;
    return write_mesh(path, xyz, nrm, NULL, nv, tri, nt, binary);
}

int oslam_ply_write_mesh_colour(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t nv,
                                const uint32_t *tri, size_t nt, int binary)
{
    static const uint8_t none[3] = {0, 0, 0};
    if (!path || (nv && (!xyz || !nrm || !rgb)) || (nt && !tri)) return OSLAM_E_INVALID;
    return write_mesh(path, xyz, nrm, rgb ? rgb : none, nv, tri, nt, binary);
}

/* the two mesh writers (rgb given: with colour) after their NULL checks */
static int write_mesh(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t nv, const uint32_t *tri,
                      size_t nt, int binary)
{
    FILE *f;
    size_t t;
    int k;
    for (t = 0; t < 3 * nt; t++)
        if (tri[t] >= nv || tri[t] > 0x7fffffffu) return OSLAM_E_INVALID;      /* the list's entries are int */
    f = fopen(path, "wb");
    if (!f) return OSLAM_E_INVALID;
    ply_header(f, binary, nv, nt, rgb != NULL);
    ply_vertices(f, binary, xyz, nrm, rgb, nv);
    for (t = 0; t < nt; t++) {
        if (binary) {
            const unsigned char three = 3;
            int32_t idx[3];
            for (k = 0; k < 3; k++) idx[k] = (int32_t)tri[3 * t + k];
            fwrite(&three, 1, 1, f);
            fwrite(idx, sizeof(int32_t), 3, f);
        } else {
            fprintf(f, "3 %u %u %u\n", tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]);
        }
    }
    return fclose(f) ? OSLAM_E_INVALID : OSLAM_OK;
}

/* ---- meshes, with or without normals (include/oslam.h at oslam_ply_read_mesh) ---- */
#define MAX_ELEMS 8
typedef struct { int is_list, slot; char ctype[16], type[16]; } mesh_prop;      /* slot: 0..5 = x y z nx ny nz, 6 = the
                                                                                    face's index list, -1 = skipped */
typedef struct { char name[32]; size_t count; int nprop; mesh_prop p[MAX_PROPS]; } mesh_elem;

/* the next value of type t: a number of the text, or the bytes of a binary file */
static int next_value(FILE *f, int ascii, const char *t, double *out)
{
    unsigned char b[8];
    if (ascii) return fscanf(f, "%lf", out) == 1;
    if (fread(b, (size_t)type_size(t), 1, f) != 1) return 0;
    *out = read_scalar(b, t);
    return 1;
}

static int is_float_type(const char *t)
{
    return !strcmp(t, "float") || !strcmp(t, "float32") || !strcmp(t, "double") || !strcmp(t, "float64");
}

int oslam_ply_read_mesh(const char *path, float **xyz_out, float **nrm_out, uint32_t **tri_out, size_t *nv_out, size_t *nt_out)
{
    static const char *names[6][2] = {{"x", "x"}, {"y", "y"}, {"z", "z"}, {"nx", "normal_x"}, {"ny", "normal_y"},
                                      {"nz", "normal_z"}};
    FILE *f;
    char line[1024];
    mesh_elem *el = NULL, *cur = NULL;
    int n_el = 0, ascii = -1, have[6] = {0, 0, 0, 0, 0, 0}, with_nrm, e, i, rc = OSLAM_E_INVALID;
    size_t nv = 0, nt = 0, cap = 0, k, j;
    float *xyz = NULL, *nrm = NULL;
    uint32_t *tri = NULL;
    if (!path || !xyz_out || !nrm_out || !tri_out || !nv_out || !nt_out) return OSLAM_E_INVALID;
    *xyz_out = *nrm_out = NULL;
    *tri_out = NULL;
    *nv_out = *nt_out = 0;
    f = fopen(path, "rb");
    if (!f) return OSLAM_E_INVALID;
    el = (mesh_elem *)calloc(MAX_ELEMS, sizeof *el);
    if (!el) { rc = OSLAM_E_NOMEM; goto done; }
    if (!fgets(line, sizeof line, f) || strncmp(line, "ply", 3)) goto done;
    while (fgets(line, sizeof line, f)) {
        char a[64] = "", b[64] = "", c[64] = "", d[64] = "", g[64] = "";
        int kk = sscanf(line, "%63s %63s %63s %63s %63s", a, b, c, d, g);
        if (kk < 1) continue;
        if (!strcmp(a, "end_header")) break;
        if (!strcmp(a, "format")) {
            if (!strcmp(b, "ascii")) ascii = 1;
            else if (!strcmp(b, "binary_little_endian")) ascii = 0;
            else goto done;
        } else if (!strcmp(a, "element")) {
            if (n_el == MAX_ELEMS) goto done;
            cur = &el[n_el++];
            snprintf(cur->name, sizeof cur->name, "%.31s", b);
            cur->count = (size_t)strtoull(c, NULL, 10);
            if ((n_el == 1) != !strcmp(b, "vertex")) goto done;      /* the vertices come first, once */
        } else if (!strcmp(a, "property")) {
            mesh_prop *p;
            if (!cur || cur->nprop == MAX_PROPS) goto done;
            p = &cur->p[cur->nprop++];
            p->slot = -1;
            if (!strcmp(b, "list")) {
                if (!type_size(c) || !type_size(d) || is_float_type(c)) goto done;
                p->is_list = 1;
                snprintf(p->ctype, sizeof p->ctype, "%.15s", c);
                snprintf(p->type, sizeof p->type, "%.15s", d);
                if (!strcmp(cur->name, "face") && (!strcmp(g, "vertex_indices") || !strcmp(g, "vertex_index"))) {
                    if (is_float_type(d)) goto done;
                    p->slot = 6;
                }
            } else {
                if (!type_size(b)) goto done;
                snprintf(p->type, sizeof p->type, "%.15s", b);
                if (cur == &el[0])
                    for (i = 0; i < 6; i++)
                        if (!strcmp(c, names[i][0]) || !strcmp(c, names[i][1])) { p->slot = i; have[i] = 1; }
            }
        }
    }
    if (ascii < 0 || n_el == 0 || !(have[0] && have[1] && have[2])) goto done;
    with_nrm = have[3] && have[4] && have[5];
    nv = el[0].count;
    xyz = (float *)malloc(sizeof(float) * 3 * (nv ? nv : 1));
    if (with_nrm) nrm = (float *)malloc(sizeof(float) * 3 * (nv ? nv : 1));
    if (!xyz || (with_nrm && !nrm)) { rc = OSLAM_E_NOMEM; goto done; }
    for (e = 0; e < n_el; e++) {
        const mesh_elem *E = &el[e];
        for (k = 0; k < E->count; k++)
            for (i = 0; i < E->nprop; i++) {
                const mesh_prop *p = &E->p[i];
                double v, first = 0.0, prev = 0.0;
                size_t cnt;
                if (!p->is_list) {
                    if (!next_value(f, ascii, p->type, &v)) goto done;
                    if (p->slot >= 0 && p->slot < 3) xyz[3 * k + p->slot] = (float)v;
                    else if (p->slot >= 3 && with_nrm) nrm[3 * k + p->slot - 3] = (float)v;
                    continue;
                }
                if (!next_value(f, ascii, p->ctype, &v) || v < 0.0) goto done;
                cnt = (size_t)v;
                for (j = 0; j < cnt; j++) {
                    if (!next_value(f, ascii, p->type, &v)) goto done;
                    if (p->slot != 6) continue;
                    if (!(v >= 0.0) || !(v < (double)nv)) goto done;              /* an index outside the vertices */
                    if (j == 0) first = v;
                    if (j >= 2) {                                                  /* the fan (0, j - 1, j) */
                        if (nt == cap) {
                            uint32_t *t2;
                            cap = cap ? 2 * cap : (E->count > 1024 ? E->count : 1024);
                            t2 = (uint32_t *)realloc(tri, sizeof(uint32_t) * 3 * cap);
                            if (!t2) { rc = OSLAM_E_NOMEM; goto done; }
                            tri = t2;
                        }
                        tri[3 * nt] = (uint32_t)first;
                        tri[3 * nt + 1] = (uint32_t)prev;
                        tri[3 * nt + 2] = (uint32_t)v;
                        nt++;
                    }
                    prev = v;
                }
            }
    }
    *xyz_out = xyz;
    *nrm_out = nrm;
    *tri_out = nt ? tri : NULL;
    if (!nt) free(tri);
    *nv_out = nv;
    *nt_out = nt;
    xyz = nrm = NULL;
    tri = NULL;
    rc = OSLAM_OK;
done:
    free(xyz);
    free(nrm);
    free(tri);
    free(el);
    fclose(f);
    return rc;
}

void oslam_free(void *p) { free(p); }
