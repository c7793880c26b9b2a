/*
 * TEST INFRASTRUCTURE ONLY.  What the reference's src/display_func.c needs from <GL/glew.h>,
 * <GL/glut.h>, <cuda_runtime.h> and <cuda_gl_interop.h> to compile as plain C with no OpenGL and
 * no CUDA (Makefile target oracle/_ref/libref_host.so): the four headers of those names in this
 * directory include this file.  Every drawing and interop call expands to nothing; only the
 * functions that compute (ReadScene, UpdateCamera, KeyFunc, SpecialFunc) are ever called.
 */
#ifndef BDPT_REF_HOST_STUB_H
#define BDPT_REF_HOST_STUB_H

typedef unsigned int GLuint;
typedef struct { unsigned char x, y, z, w; } uchar4;
typedef int cudaError_t;
#define cudaSuccess 0
#define cudaGetErrorString(e) "no CUDA"
#define cudaGLMapBufferObject(...) cudaSuccess
#define cudaGLUnmapBufferObject(...) cudaSuccess

/* GLUT's special-key codes (freeglut_std.h) and the one font handle passed to a real function */
#define GLUT_KEY_LEFT 100
#define GLUT_KEY_UP 101
#define GLUT_KEY_RIGHT 102
#define GLUT_KEY_DOWN 103
#define GLUT_KEY_PAGE_UP 104
#define GLUT_KEY_PAGE_DOWN 105
#define GLUT_BITMAP_HELVETICA_18 ((void *)0)

#define glewInit(...) ((void)0)
#define glewIsSupported(...) 1
#define glutBitmapCharacter(...) ((void)0)
#define glutPostRedisplay(...) ((void)0)
#define glutSwapBuffers(...) ((void)0)
#define glutInit(...) ((void)0)
#define glutInitDisplayMode(...) ((void)0)
#define glutInitWindowSize(...) ((void)0)
#define glutCreateWindow(...) ((void)0)
#define glutReshapeFunc(...) ((void)0)
#define glutKeyboardFunc(...) ((void)0)
#define glutSpecialFunc(...) ((void)0)
#define glutDisplayFunc(...) ((void)0)
#define glutIdleFunc(...) ((void)0)
#define glEnable(...) ((void)0)
#define glDisable(...) ((void)0)
#define glBlendFunc(...) ((void)0)
#define glColor3f(...) ((void)0)
#define glColor4f(...) ((void)0)
#define glRecti(...) ((void)0)
#define glRasterPos2i(...) ((void)0)
#define glBindBuffer(...) ((void)0)
#define glBindTexture(...) ((void)0)
#define glClear(...) ((void)0)
#define glClearColor(...) ((void)0)
#define glTexSubImage2D(...) ((void)0)
#define glBegin(...) ((void)0)
#define glEnd(...) ((void)0)
#define glTexCoord2f(...) ((void)0)
#define glVertex3f(...) ((void)0)
#define glPushMatrix(...) ((void)0)
#define glPopMatrix(...) ((void)0)
#define glLoadIdentity(...) ((void)0)
#define glMatrixMode(...) ((void)0)
#define glOrtho(...) ((void)0)
#define glViewport(...) ((void)0)
#define glFlush(...) ((void)0)

#endif
