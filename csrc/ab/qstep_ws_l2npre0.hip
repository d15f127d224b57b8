// A/B build of csrc/qstep_ws.hip: Q(x')'s layer 2 reads all its W1 fragments inside the phase (the form before WS_L2NPRE).
#define WS_L2NPRE 0
#define WS_NS ws_l2npre0
#define WS_API(name) name##_l2npre0
#include "../qstep_ws.hip"
