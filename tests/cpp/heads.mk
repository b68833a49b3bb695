# tests/cpp/heads.mk — TEST CODE: the host simulations of the heads of sparse attention in one call, built beside the
# programs of tests/cpp/Makefile by its one rule and its SIM_SAN flags (make -C tests/cpp -f heads.mk TARGET):
#   attention_heads_sim      csrc/attention.hip through _reserve_heads / _execute_heads / _execute:
#                            tests/test_attention_heads_sim_cpu.py
#   attention_bwd_heads_sim  csrc/attention_bwd.hip (beside csrc/coo_csr.hip) through the same entry points of the backward
#                            object: tests/test_attention_bwd_heads_sim_cpu.py
include Makefile

HEADS_SIMS := attention_heads_sim attention_bwd_heads_sim
attention_heads_sim: $(CSRC)/attention.hip $(CSRC)/attention_common.hpp $(CSRC)/attention_slice_walk.inc $(CSRC)/attention_half_kernel.hpp sim_operand.hpp sim_heads.hpp
attention_bwd_heads_sim: $(CSRC)/attention_bwd.hip $(CSRC)/attention_common.hpp $(CSRC)/attention_bwd_slice_walk.inc $(CSRC)/attention_bwd_half_kernel.hpp \
                         $(CSRC)/coo_csr.hip sim_runtime.hpp sim_operand.hpp sim_heads.hpp
$(HEADS_SIMS): %: %.cpp $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<

clean: clean_heads
clean_heads:
	rm -f $(HEADS_SIMS)
.PHONY: clean_heads
