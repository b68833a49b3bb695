# tests/cpp/multi_semiring_sim.mk — TEST CODE: the rule of multi_semiring_sim (tests/test_multi_semiring_sim_cpu.py), over
# the Makefile's own variables and sanitizer flags (SIM_SAN):   make -C tests/cpp -f multi_semiring_sim.mk multi_semiring_sim
include Makefile

multi_semiring_sim: multi_semiring_sim.cpp simt/hip/hip_runtime.h $(CSRC)/multi.hip $(CSRC)/multi_kernels.hpp $(CSRC)/semiring.hpp \
                    $(CSRC)/common.hpp ../../include/mi355_spmv.h
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ multi_semiring_sim.cpp

# multi.hip includes these two headers; the Makefile's multi_sim rule lists only multi.hip and common.hpp.  Through this
# fragment multi_sim is rebuilt after an edit to them as well (prerequisites added to the Makefile's rule).
multi_sim: $(CSRC)/multi_kernels.hpp $(CSRC)/semiring.hpp
