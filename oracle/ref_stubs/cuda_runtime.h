/* Empty stand-in: see ref_host_stub.h. */
#include "ref_host_stub.h"
