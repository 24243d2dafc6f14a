// pk_error.cpp -- fail(): the error message of a call, in its context or (no context) in the calling thread's slot.
#include "pk_error.h"

#include <cstdarg>
#include <cstdio>

namespace {
thread_local std::string g_create_error;
}

int fail(pk_error_state* c, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->error = buf; else g_create_error = buf;
  return code;
}

const char* last_contextless_error() { return g_create_error.c_str(); }
