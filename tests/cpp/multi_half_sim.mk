# tests/cpp/multi_half_sim.mk — TEST CODE: the rule of multi_half_sim (tests/test_multi_half_sim_cpu.py), over the
# Makefile's own variables and sanitizer flags (SIM_SAN):   make -C tests/cpp -f multi_half_sim.mk multi_half_sim
include Makefile

SIM_HDRS := simt/hip/hip_runtime.h $(CSRC)/multi.hip $(CSRC)/multi_kernels.hpp $(CSRC)/multi_half_kernels.hpp $(CSRC)/semiring.hpp \
            $(CSRC)/common.hpp ../../include/mi355_spmv.h

multi_half_sim: multi_half_sim.cpp $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ multi_half_sim.cpp

# multi.hip includes these headers; the Makefile's own rules for the two older programs do not list them all.  Through
# this fragment they are rebuilt after an edit to any of them (prerequisites added to the Makefile's rules; the recipe
# of multi_semiring_sim is that of multi_semiring_sim.mk).
multi_sim: $(SIM_HDRS)
multi_semiring_sim: multi_semiring_sim.cpp $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ multi_semiring_sim.cpp
