# tests/sim/projection.mk -- TEST AID built by tests/test_projection_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_projection.so = the objects of libmvo_sim_epipolar.so (epipolar.mk) plus
# csrc/projection_host.cpp and csrc/projection_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule:
# every lane of k_map_match_projection runs as a fiber on the CPU.
#   make -C tests/sim -f projection.mk _build/libmvo_sim_projection.so
include epipolar.mk
PROJECTION_OBJ := $(EPIPOLAR_OBJ) _build/full/projection_host.cpp.o _build/full/projection_kernels.hip.o
_build/libmvo_sim_projection.so: $(PROJECTION_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
