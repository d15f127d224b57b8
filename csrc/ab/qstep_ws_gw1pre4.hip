// A/B build of csrc/qstep_ws.hip: the gradient waves read all of dZ1's W1^T fragments (four k-steps, 32 VGPRs) before the
// wait for the slot pair (256 VGPRs; ties with none read ahead).
#define WS_GW1PRE 4
#define WS_NS ws_gw1pre4
#define WS_API(name) name##_gw1pre4
#include "../qstep_ws.hip"
