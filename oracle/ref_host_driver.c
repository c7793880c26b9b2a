/*
 * TEST INFRASTRUCTURE ONLY: the host side of oracle/_ref/libref_host.so.
 *
 * libref_host.so is the reference's own src/display_func.c compiled in place as C (the language
 * of the file: `sqrt` in vec.h's vnorm is the double libm sqrt there) against the empty GL/CUDA
 * stand-ins of oracle/ref_stubs/.  This file owns the globals display_func.c expects from
 * smallpt_cpu.c (camera, spheres, sphereCount, ...) and the entry points it calls back: ReInit
 * and ReInitScene only count their calls -- in the reference they re-derive the camera and
 * restart the render (smallpt_cpu.c:365-387), which the tests do explicitly.
 */
#include <stdlib.h>
#include <string.h>

#include <cuda_runtime.h>
#include <GL/glew.h>

#include "camera.h"
#include "geom.h"

Camera camera;
Sphere *spheres;
unsigned int sphereCount;
GLuint pbo, textureID;
uchar4 *pixels_buf;
int allFlag;

extern int width, height;
extern void ReadScene(char *);
extern void UpdateCamera();
extern void KeyFunc(unsigned char key, int x, int y);
extern void SpecialFunc(int key, int x, int y);

static int n_reinit, n_reinit_scene, last_realloc;
static unsigned current;           /* shadow of display_func.c's static currentSphere (:59,336,342) */

void ReInit(const int reallocBuffers) { n_reinit++; last_realloc = reallocBuffers; }
void ReInitScene(void) { n_reinit_scene++; }
void UpdateRendering2(void) {}
void UpdateRendering(void) {}
void SavePPM(int number) { (void)number; }

/* KeyFunc; returns (ReInit calls) | (ReInitScene calls) << 8 made by the key. */
int refhost_key(int key)
{
    const int a = n_reinit, b = n_reinit_scene;
    if (sphereCount) {
        if (key == '+') current = (current + 1) % sphereCount;
        if (key == '-') current = (current + (sphereCount - 1)) % sphereCount;
    }
    KeyFunc((unsigned char)key, 0, 0);
    return (n_reinit - a) | ((n_reinit_scene - b) << 8);
}

int refhost_special(int key)
{
    const int a = n_reinit, b = n_reinit_scene;
    SpecialFunc(key, 0, 0);
    return (n_reinit - a) | ((n_reinit_scene - b) << 8);
}

int refhost_last_realloc(void) { return last_realloc; }
unsigned refhost_current_sphere(void) { return current; }

/* currentSphere is private to display_func.c: bring it back to 0 with the '+' key itself. */
static void select_zero(void)
{
    while (sphereCount && current != 0) refhost_key('+');
}

/* ReadScene (exits on a malformed file: only given files that exist); returns sphereCount. */
unsigned refhost_read_scene(const char *path)
{
    select_zero();
    free(spheres);
    spheres = NULL;
    sphereCount = 0;
    memset(&camera, 0, sizeof camera);
    char *p = strdup(path);
    ReadScene(p);
    free(p);
    return sphereCount;
}

void refhost_get_camera(Camera *out) { *out = camera; }
void refhost_set_camera(const Camera *in) { camera = *in; }
void refhost_get_spheres(Sphere *out) { memcpy(out, spheres, sizeof(Sphere) * sphereCount); }

/* UpdateCamera at the given internal frame size (width/height are display_func.c's globals). */
void refhost_update_camera(int w, int h)
{
    width = w;
    height = h;
    UpdateCamera();
}
