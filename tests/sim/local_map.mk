# tests/sim/local_map.mk -- TEST AID built by tests/test_local_map_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_local_map.so = the objects of libmvo_sim_projection.so (projection.mk) plus
# csrc/local_map_host.cpp and csrc/local_map_kernels.hip, compiled for x86 against hip_emu/ by the same pattern rule:
# every lane of k_map_match_local runs as a fiber on the CPU.
#   make -C tests/sim -f local_map.mk _build/libmvo_sim_local_map.so
include projection.mk
LOCAL_MAP_OBJ := $(PROJECTION_OBJ) _build/full/local_map_host.cpp.o _build/full/local_map_kernels.hip.o
_build/libmvo_sim_local_map.so: $(LOCAL_MAP_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
