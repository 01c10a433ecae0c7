/*
 * oracle/ref_shim/windows.h -- the few Win32 names the reference's headers use
 * outside its window code (which oracle/ref_build.py does not compile).
 * TEST INFRASTRUCTURE ONLY.
 */
#ifndef REF_SHIM_WINDOWS_H
#define REF_SHIM_WINDOWS_H

#include "cuda_runtime.h" /* every standard header first: min / max below are macros */

typedef void* HWND;

/* virtual-key codes (winuser.h) */
#define VK_RETURN 0x0D
#define VK_ESCAPE 0x1B
#define VK_LEFT 0x25
#define VK_UP 0x26
#define VK_RIGHT 0x27
#define VK_DOWN 0x28
#define VK_F1 0x70

/* minwindef.h */
#ifndef max
#define max(a, b) (((a) > (b)) ? (a) : (b))
#endif
#ifndef min
#define min(a, b) (((a) < (b)) ? (a) : (b))
#endif

#endif
