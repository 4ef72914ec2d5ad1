# tests/sim/orb_distribute.mk -- TEST AID built by tests/test_orb_distribute_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_orb_distribute.so = the objects of libmvo_sim_projection.so (projection.mk) plus
# csrc/orb_distribute_host.cpp and csrc/orb_distribute_kernels.hip, compiled for x86 against hip_emu/ by the same pattern
# rule: every lane of k_fast_cells and k_ic_angle runs as a fiber on the CPU.
#   make -C tests/sim -f orb_distribute.mk _build/libmvo_sim_orb_distribute.so
include projection.mk
ORB_DISTRIBUTE_OBJ := $(PROJECTION_OBJ) _build/full/orb_distribute_host.cpp.o _build/full/orb_distribute_kernels.hip.o
_build/libmvo_sim_orb_distribute.so: $(ORB_DISTRIBUTE_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
_build/full/orb_kernels.hip.o _build/full/orb_distribute_kernels.hip.o: $(CSRC)/orb_device.h
