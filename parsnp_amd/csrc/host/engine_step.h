// engine_step.h -- what the steps beside the XMFA (snps.cpp, tree.cpp, recomb.cpp, extend.cpp) do around every call of the engine
#pragma once
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include "../../../include/parsnp_mum.h"

namespace parsnp {
// kernel time of the session's last call (pm_last_timing): the phases called `name`, or, with `prefix`, those whose names begin with it
inline double phase_ms(const pm_session* s, const char* name, bool prefix) {
    int cnt = 64; const char* names[64]; float ms[64];
    if (pm_last_timing(s, &cnt, names, ms) != PM_OK) return 0;
    double sum = 0;
    for (int i = 0; i < cnt; i++) if (prefix ? !strncmp(names[i], name, strlen(name)) : !strcmp(names[i], name)) sum += ms[i];
    return sum;
}
// a call that failed ends the run: exit code 5 when the input exceeds a limit of the engine, 1 otherwise
inline void engine_check(int rc, const std::string& what) {
    if (rc == PM_OK) return;
    std::cerr << "parsnp_core: " << what << ": " << pm_last_error() << std::endl;
    exit(rc == PM_ELIMIT ? 5 : 1);
}
}  // namespace parsnp
