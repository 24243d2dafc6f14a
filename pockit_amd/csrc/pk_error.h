// pk_error.h -- where the runtime keeps the message of a failed call (pk_last_error).  Free of HIP: the helper-thread pool
// (pk_pool.cpp) needs nothing else of the runtime.
#ifndef PK_ERROR_H
#define PK_ERROR_H

#include <string>

// the part of pk_ctx (its base) that fail() writes
struct pk_error_state {
  std::string error;
};

#pragma GCC visibility push(hidden)      // (internal to the library)

// Records the formatted message in the context -- c == nullptr: in the calling thread's slot for calls without a context
// (pk_create, pk_host_alloc, pk_host_threads, ...) -- and returns `code`.
int fail(pk_error_state* c, int code, const char* fmt, ...);

// the message of the last fail(nullptr, ...) of this thread
const char* last_contextless_error();

#pragma GCC visibility pop
#endif  // PK_ERROR_H
