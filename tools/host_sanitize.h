/* host_sanitize.h -- what the stand-alone sanitizer drivers of the host
 * validators share (tools/*_host_sanitize.c): the failure count, expect()
 * and refused().  A driver returns 1 from main when `failures` is non-zero. */
#ifndef HOST_SANITIZE_H
#define HOST_SANITIZE_H

#include <stdio.h>
#include <string.h>

#include "gsplat_hip.h"

static int failures = 0;

static void expect(int ok, const char *what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s (last error: %s)\n", what, gs_last_error());
    ++failures;
  }
}

/* a validator's return `code` is an error whose message contains `needle` */
static int refused(int code, const char *needle) {
  return code < 0 && strstr(gs_last_error(), needle) != NULL;
}

#endif
