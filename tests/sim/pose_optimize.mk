# tests/sim/pose_optimize.mk -- TEST AID built by tests/test_pose_optimize_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_pose_optimize.so = the objects of libmvo_sim_window_triangulate.so (window_triangulate.mk) plus
# csrc/pose_optimize_host.cpp and csrc/pose_optimize_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule:
# every lane of k_pose_optimize runs as a fiber on the CPU, its __shfl_xor levels and its barriers included.
#   make -C tests/sim -f pose_optimize.mk _build/libmvo_sim_pose_optimize.so
include window_triangulate.mk
POSE_OPTIMIZE_OBJ := $(WINDOW_TRIANGULATE_OBJ) _build/full/pose_optimize_host.cpp.o _build/full/pose_optimize_kernels.hip.o
_build/full/pose_optimize_kernels.hip.o: $(CSRC)/pnp_wave.h
_build/libmvo_sim_pose_optimize.so: $(POSE_OPTIMIZE_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
