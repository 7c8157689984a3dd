// tu_3d_env.hip -- translation unit of the Cassie3d environment layer (cassie3d_env.hip).
#include "cassie3d_env.hip"
