// Time stepping of the facade: TimeSteppingTools, TimeProblem, DAESolverInTime -- the subsets the reference's unsteadyLinElas
// and unsteadyNavierStokes tests run (feddlib/problems/tests/unsteadyLinElas/main.cpp, unsteadyNavierStokes/main.cpp):
// "Newmark" on a linear one-block problem, and "Multistep" (BDF1 / BDF2) on Navier-Stokes (two variables, time definition
// [[1,1],[0,0]]); one rank.
//   TimeSteppingTools   feddlib/problems/Solver/TimeSteppingTools.cpp (the keys the Newmark path reads)
//   TimeProblem         feddlib/problems/abstract/TimeProblem_def.hpp (assembleMassSystem :599-663, combineSystems :359-408,
//                       updateNewmarkRhs :473-524, updateSolutionNewmarkPreviousStep :875-981)
//                       nonlinear: updateSolutionMultiPreviousStep :833-849, updateMultistepRhs :417-438,
//                       calculateNonLinResidualVec :693-738, setBoundariesSystem / solveUpdate / solveAndUpdate :767-803
//   DAESolverInTime     feddlib/problems/Solver/DAESolverInTime_def.hpp (advanceInTimeLinearNewmark :519-607,
//                       advanceInTimeNonLinearMultistep :1209-1333)
//   NonLinearSolver::solve(TimeProblem&, time)   NonLinearSolver_def.hpp:394-531
//   nonlinear Newmark: "Newmark" on NonLinElasticity (1 x 1 definition, Newton) -- advanceInTimeNonLinearNewmark :613-722; the
//                       Newton iterate, residual and update stay on the device (fedd_assemble_hyperelastic_time, fedd_newton_*),
//                       the host vectors of the facade are refreshed once per step
// Everything else these classes do in the reference (single-step / Butcher-table schemes, adaptive steps, "Extrapolation", NOX,
// source terms in the multistep loop, FSI) is an error here that names what is built.
#pragma once
#include "fedd_facade.hpp"

namespace FEDD {

// the square matrix of small size the reference passes time-stepping definitions and coefficients in (SmallMatrix.hpp)
template <class T>
class SmallMatrix {
public:
    SmallMatrix() : n_(0) {}
    explicit SmallMatrix(int n) : n_(n), v_((size_t)n, std::vector<T>((size_t)n, T())) {}
    SmallMatrix(int n, T value) : n_(n), v_((size_t)n, std::vector<T>((size_t)n, value)) {}
    std::vector<T>& operator[](int i) { return v_.at((size_t)i); }
    const std::vector<T>& operator[](int i) const { return v_.at((size_t)i); }
    int size() const { return n_; }
private:
    int n_;
    std::vector<std::vector<T>> v_;
};

class TimeSteppingTools {
public:
    TimeSteppingTools(ParameterListPtr_Type parameterList, Teuchos::RCP<const Teuchos::Comm<int>> comm)
        : pl_(parameterList), comm_(comm) {
        // (the constructor is handed the "Timestepping Parameter" sublist, as in the reference)
        const std::string type = pl_->get("Timestepping type", "non-adaptive");
        TEUCHOS_TEST_FOR_EXCEPTION(type != "non-adaptive", std::logic_error,
                                   "Timestepping type \"" + type + "\" is not built (\"non-adaptive\" is)");
        class_ = pl_->get("Class", "Newmark");
        dt_ = pl_->get("dt", 0.01);
        tEnd_ = pl_->get("Final time", 1.);
        beta_ = pl_->get("beta", 0.25);
        gamma_ = pl_->get("gamma", 0.5);
        TEUCHOS_TEST_FOR_EXCEPTION(dt_ <= 0., std::logic_error, "Timestepping Parameter: dt must be positive");
        bdf_ = pl_->get("BDF", 1);
        if (class_ == "Multistep") checkBDF();
    }
    // TimeSteppingTools.cpp:493-515: {M u_new / dt, A u_new, M u_n / dt (, M u_{n-1} / dt)}
    int getBDFNumber() const { checkBDF(); return bdf_; }
    double getInformationBDF(int i) const {
        checkBDF();
        static const double one[3] = {1., 1., 1.}, two[4] = {1.5, 1.0, 2.0, -0.5};
        TEUCHOS_TEST_FOR_EXCEPTION(i < 0 || i + 1 > bdf_ + 2, std::logic_error, "Wrong bdf table access!");
        return bdf_ == 1 ? one[i] : two[i];
    }
    std::string getClass() const { return class_; }
    double get_dt() const { return dt_; }
    double get_beta() const { return beta_; }
    double get_gamma() const { return gamma_; }
    double currentTime() const { return t_; }
    int currentStep() const { return step_; }
    bool continueTimeStepping() const { return t_ + 1.e-10 < tEnd_; }       // TimeSteppingTools.cpp: t < tEnd with the same slack
    void advanceTime(bool printInfo = false) {
        t_ += dt_;
        ++step_;
        if (printInfo && comm_->getRank() == 0) std::cout << "-- time step " << step_ << " done, t = " << t_ << " --" << std::endl;
    }
private:
    void checkBDF() const {
        TEUCHOS_TEST_FOR_EXCEPTION(bdf_ != 1 && bdf_ != 2, std::logic_error,
                                   "Timestepping Parameter \"BDF\" = " + std::to_string(bdf_) + " is not built (1 and 2 are)");
    }
    ParameterListPtr_Type pl_;
    Teuchos::RCP<const Teuchos::Comm<int>> comm_;
    int bdf_ = 1;
    std::string class_;
    double dt_ = 0., tEnd_ = 0., beta_ = 0.25, gamma_ = 0.5, t_ = 0.;
    int step_ = 0;
};

// Wraps a linear single-block Problem.  The mass matrix lives in device slot 0, the problem's matrix in slot 1, the combined
// matrix is the device's system matrix; u_n, v, w live on the device (fedd_newmark_*); right-hand side, source term and
// solution are the wrapped problem's host vectors, as everywhere in this facade.
template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class TimeProblem {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef typename Problem_Type::Matrix_Type Matrix_Type;
    typedef typename Problem_Type::MatrixPtr_Type MatrixPtr_Type;
    typedef typename Problem_Type::BlockMatrix_Type BlockMatrix_Type;
    typedef typename Problem_Type::BlockMatrixPtr_Type BlockMatrixPtr_Type;
    typedef typename Problem_Type::BlockMultiVectorPtr_Type BlockMultiVectorPtr_Type;
    typedef Teuchos::RCP<const Teuchos::Comm<int>> CommConstPtr_Type;
    typedef NonLinearProblem<SC, LO, GO, NO> NonLinearProblem_Type;
    typedef NavierStokes<SC, LO, GO, NO> NavierStokes_Type;
    typedef NonLinElasticity<SC, LO, GO, NO> NonLinElasticity_Type;
    static constexpr int SLOT_MASS = 0, SLOT_SYSTEM = 1;
    // nonlinear path (Navier-Stokes occupies slots 0 .. 4): velocity mass, time-combined constant velocity block
    static constexpr int SLOT_NL_A = 0, SLOT_NL_MASS = 5, SLOT_NL_COMBINED = 6;

    TimeProblem(Problem_Type& problem, CommConstPtr_Type comm) : problem_(&problem), comm_(comm) {
        TEUCHOS_TEST_FOR_EXCEPTION(comm->getSize() != 1, std::logic_error, "TimeProblem: one rank only (the time-stepping device layer is one rank)");
        nl_ = dynamic_cast<NonLinearProblem_Type*>(problem_);
        ns_ = dynamic_cast<NavierStokes_Type*>(problem_);
        nle_ = dynamic_cast<NonLinElasticity_Type*>(problem_);
        TEUCHOS_TEST_FOR_EXCEPTION(nl_ != nullptr && ns_ == nullptr && nle_ == nullptr, std::logic_error,
                                   "TimeProblem: NavierStokes (\"Multistep\") and NonLinElasticity (\"Newmark\") are the nonlinear problems that are built");
        // the BDF layer combines the DIAG velocity mass (slot 5) and A (slot 0) as two DIAG matrices; with the stress form A is FULL
        TEUCHOS_TEST_FOR_EXCEPTION(ns_ != nullptr && problem_->getParameterList()->sublist("Parameter").get("Symmetric gradient", false),
                                   std::logic_error,
                                   "TimeProblem: \"Symmetric gradient\" = true is refused in the time loop: steady Stokes is the problem that assembles the "
                                   "stress form; Navier-Stokes and its time loop take the vector Laplacian (set the key to false)");
    }
    bool isNonLinear() const { return nl_ != nullptr; }
    bool isNonLinElasticity() const { return nle_ != nullptr; }
    void setTimeDef(const SmallMatrix<int>& def) {
        if (nle_) {
            TEUCHOS_TEST_FOR_EXCEPTION(def.size() != 1 || def[0][0] != 1, std::logic_error,
                                       "TimeProblem::setTimeDef: NonLinElasticity takes the 1 x 1 definition [[1]] (one block, \"Newmark\"); a " +
                                           std::to_string(def.size()) + " x " + std::to_string(def.size()) + " definition is not built");
        } else if (nl_) {
            TEUCHOS_TEST_FOR_EXCEPTION(def.size() != 2 || def[0][0] != 1 || def[0][1] != 1 || def[1][0] != 0 || def[1][1] != 0, std::logic_error,
                                       "TimeProblem::setTimeDef: a nonlinear problem takes the 2 x 2 definition [[1,1],[0,0]] (velocity, pressure)");
        } else {
            TEUCHOS_TEST_FOR_EXCEPTION(def.size() != 1, std::logic_error, "TimeProblem::setTimeDef: only a 1 x 1 definition is built (one block, \"Newmark\")");
        }
        timeStepDef_ = def;
    }
    // TimeProblem::assembleMassSystem (:599-663): FE::assemblyMass on the variable's space, scaled by "Density" (:605, 620).
    // The problem's own matrix, still in the device's system slot after Problem::assemble, moves to slot 1 first.
    void assembleMassSystem() {
        if (nle_) {     // the mass as the linear Newmark path assembles it, with "Density", into slot 0; the FULL pattern goes back into the system slot
            dev_ = problem_->getDomain(0)->device();
            const int dim = (int)problem_->getDomain(0)->getDimension();
            const double density = problem_->getParameterList()->sublist("Parameter").get("Density", 1.);
            MatrixPtr_Type M = Teuchos::rcp(new Matrix_Type(problem_->getDomain(0)->getMapVecFieldUnique(), problem_->getDomain(0)->getApproxEntriesPerRow()));
            problem_->getFEFactory()->assemblyMass(dim, problem_->getFEType(0), "Vector", M);
            M->scale(density);
            feddCheck(fedd_matrix_store(dev_->ctx, SLOT_MASS), "fedd_matrix_store");
            M->bindSlot(dev_, SLOT_MASS);
            systemMass_.reset(new BlockMatrix_Type(1));
            systemMass_->addBlock(M, 0, 0);
            nle_->restorePattern();
            return;
        }
        if (nl_) {      // the vector mass on the velocity space x "Density" into slot 5; the system slot is scratch until the next reAssemble
            dev_ = problem_->getDomain(0)->device();
            const int dim = (int)problem_->getDomain(0)->getDimension();
            const double density = problem_->getParameterList()->sublist("Parameter").get("Density", 1.);
            MatrixPtr_Type M = Teuchos::rcp(new Matrix_Type(problem_->getDomain(0)->getMapVecFieldUnique(), problem_->getDomain(0)->getApproxEntriesPerRow()));
            problem_->getFEFactory()->assemblyMass(dim, problem_->getFEType(0), "Vector", M);
            M->scale(density);
            feddCheck(fedd_matrix_store(dev_->ctx, SLOT_NL_MASS), "fedd_matrix_store");
            M->bindSlot(dev_, SLOT_NL_MASS);
            systemMass_.reset(new BlockMatrix_Type(2));
            systemMass_->addBlock(M, 0, 0);
            return;
        }
        auto sys = problem_->getSystem();
        TEUCHOS_TEST_FOR_EXCEPTION(sys.is_null() || sys->size() != 1 || !sys->blockExists(0, 0), std::logic_error,
                                   "TimeProblem: a single-block problem, assembled (Problem::assemble), is needed");
        MatrixPtr_Type K = sys->getBlock(0, 0);
        TEUCHOS_TEST_FOR_EXCEPTION(!K->isResident(), std::runtime_error, "TimeProblem: the problem's matrix is not resident on the device");
        dev_ = K->device();
        if (K->slot() < 0) {
            feddCheck(fedd_matrix_store(dev_->ctx, SLOT_SYSTEM), "fedd_matrix_store");
            K->bindSlot(dev_, SLOT_SYSTEM);
        }
        const int dofs = problem_->getDofsPerNode(0), dim = (int)problem_->getDomain(0)->getDimension();
        const double density = problem_->getParameterList()->sublist("Parameter").get("Density", 1.);
        auto map = dofs > 1 ? problem_->getDomain(0)->getMapVecFieldUnique() : problem_->getDomain(0)->getMapUnique();
        MatrixPtr_Type M = Teuchos::rcp(new Matrix_Type(map, problem_->getDomain(0)->getApproxEntriesPerRow()));
        problem_->getFEFactory()->assemblyMass(dim, problem_->getFEType(0), dofs > 1 ? "Vector" : "Scalar", M);
        M->scale(density);
        feddCheck(fedd_matrix_store(dev_->ctx, SLOT_MASS), "fedd_matrix_store");
        M->bindSlot(dev_, SLOT_MASS);
        systemMass_.reset(new BlockMatrix_Type(1));
        systemMass_->addBlock(M, 0, 0);
    }
    void setTimeParameters(const SmallMatrix<double>& massParameters, const SmallMatrix<double>& timeParameters) {
        if (nle_) {
            TEUCHOS_TEST_FOR_EXCEPTION(massParameters.size() != 1 || timeParameters.size() != 1, std::logic_error, "TimeProblem: 1 x 1 parameters only");
            TEUCHOS_TEST_FOR_EXCEPTION(timeParameters[0][0] != 1., std::logic_error,
                                       "TimeProblem::setTimeParameters: a problem coefficient other than 1.0 is not built for NonLinElasticity (Newmark gives 1.0)");
            massParameters_ = massParameters;
            timeParameters_ = timeParameters;
            return;
        }
        if (nl_) {
            TEUCHOS_TEST_FOR_EXCEPTION(massParameters.size() != 2 || timeParameters.size() != 2, std::logic_error, "TimeProblem: 2 x 2 parameters for a nonlinear problem");
            TEUCHOS_TEST_FOR_EXCEPTION(timeParameters[0][1] != 1. || timeParameters[1][0] != 1. || timeParameters[1][1] != 1., std::logic_error,
                                       "TimeProblem::setTimeParameters: off-diagonal and pressure-row problem coefficients other than 1.0 are not built (BDF gives 1.0)");
            TEUCHOS_TEST_FOR_EXCEPTION(massParameters[0][1] != 0. || massParameters[1][0] != 0. || massParameters[1][1] != 0., std::logic_error,
                                       "TimeProblem::setTimeParameters: mass coefficients outside the velocity block are not built (the time definition is [[1,1],[0,0]])");
            massParameters_ = massParameters;
            timeParameters_ = timeParameters;
            return;
        }
        TEUCHOS_TEST_FOR_EXCEPTION(massParameters.size() != 1 || timeParameters.size() != 1, std::logic_error, "TimeProblem: 1 x 1 parameters only");
        massParameters_ = massParameters;
        timeParameters_ = timeParameters;
    }
    // TimeProblem::combineSystems (:359-408) -> fedd_matrix_combine.  The reference combines in every step; here the combined
    // matrix is rebuilt only when the coefficients or either matrix changed since the last combine (same results)
    // Nonlinear: slot 6 <- (cm * M[5]) + (ca * A[0]) when (cm, ca) changed -- once per coefficient set, twice in a BDF2 run --, the
    // base slot of NavierStokes::reAssemble becomes 6, and one reAssemble puts the merged time system into the system slot.
    // The reference adds the matrices in every nonlinear iteration; the sums are the same.
    void combineSystems() {
        TEUCHOS_TEST_FOR_EXCEPTION(systemMass_.is_null(), std::logic_error, "TimeProblem::combineSystems: call assembleMassSystem first");
        const double cm = massParameters_[0][0], ca = timeParameters_[0][0];
        if (nle_) {     // the tangent changes with u: (cm M) + K(u) is formed where K(u) is, in calculateNonLinResidualVec
            ++combines_;
            return;
        }
        if (nl_) {
            if (nlCombined_ && cm == nlCm_ && ca == nlCa_) return;
            int cur = 0;
            feddCheck(fedd_matrix_combine_current(dev_->ctx, SLOT_NL_MASS, cm, SLOT_NL_A, ca, &cur), "fedd_matrix_combine_current");
            if (!cur) feddCheck(fedd_matrix_combine(dev_->ctx, SLOT_NL_MASS, cm, SLOT_NL_A, ca), "fedd_matrix_combine");
            feddCheck(fedd_matrix_store(dev_->ctx, SLOT_NL_COMBINED), "fedd_matrix_store");
            dev_->generation++;
            nlCombined_ = true; nlCm_ = cm; nlCa_ = ca;
            ++combines_;
            ns_->setVelocityBaseSlot(SLOT_NL_COMBINED);
            nl_->reAssemble("FixedPoint");
            return;
        }
        int current = 0;
        feddCheck(fedd_matrix_combine_current(dev_->ctx, SLOT_MASS, cm, SLOT_SYSTEM, ca, &current), "fedd_matrix_combine_current");
        if (current && !systemCombined_.is_null()) return;
        feddCheck(fedd_matrix_combine(dev_->ctx, SLOT_MASS, cm, SLOT_SYSTEM, ca), "fedd_matrix_combine");
        dev_->generation++;
        MatrixPtr_Type C = Teuchos::rcp(new Matrix_Type(systemMass_->getBlock(0, 0)->getMap()));
        C->bind(dev_, problem_->getDofsPerNode(0));
        systemCombined_.reset(new BlockMatrix_Type(1));
        systemCombined_->addBlock(C, 0, 0);
        fresh_ = true;
        ++combines_;
    }
    // updateSolutionNewmarkPreviousStep (:875-981) and updateNewmarkRhs (:473-524) are ONE device call, fedd_newmark_advance:
    // the first only records its arguments, the second launches (state update, then rhs <- coeff * M t) and brings the
    // right-hand side to the host vector.  Calling the second without the first is an error.
    void updateSolutionNewmarkPreviousStep(double dt, double beta, double gamma) {
        pend_ = true; pendDt_ = dt; pendBeta_ = beta; pendGamma_ = gamma;
    }
    void updateNewmarkRhs(double dt, double beta, double gamma, vec_dbl_Type coeff) {
        TEUCHOS_TEST_FOR_EXCEPTION(!pend_ || dt != pendDt_ || beta != pendBeta_ || gamma != pendGamma_, std::logic_error,
                                   "TimeProblem::updateNewmarkRhs: call updateSolutionNewmarkPreviousStep with the same dt, beta, gamma first");
        TEUCHOS_TEST_FOR_EXCEPTION(systemCombined_.is_null() && !nle_, std::logic_error, "TimeProblem::updateNewmarkRhs: call combineSystems first");
        pend_ = false;
        if (!began_) {       // the start values of :913-926: u_n <- the problem's solution, v = w = 0
            feddCheck(fedd_solution_set(dev_->ctx, problem_->getSolution()->getBlock(0)->raw().data()), "fedd_solution_set");
            feddCheck(fedd_newmark_begin(dev_->ctx), "fedd_newmark_begin");
            began_ = true;
        }
        feddCheck(fedd_newmark_advance(dev_->ctx, SLOT_MASS, dt, beta, gamma, coeff.at(0)), "fedd_newmark_advance");
        feddCheck(fedd_rhs_get(dev_->ctx, problem_->getRhs()->getBlockNonConst(0)->raw().data()), "fedd_rhs_get");
    }
    // updateSolutionMultiPreviousStep (:833-849) and updateMultistepRhs (:417-438) are ONE device call, fedd_multistep_advance:
    // the first only records, the second launches (history shift, rhs <- [M t; 0]) and brings the right-hand side to the host.
    void updateSolutionMultiPreviousStep(int nmbSteps) {
        TEUCHOS_TEST_FOR_EXCEPTION(!nl_, std::logic_error, "TimeProblem::updateSolutionMultiPreviousStep: the multistep path is built for nonlinear problems");
        pendMs_ = true; pendSteps_ = nmbSteps;
    }
    void updateMultistepRhs(vec_dbl_Type& coeff, int nmbToUse) {
        TEUCHOS_TEST_FOR_EXCEPTION(!pendMs_, std::logic_error, "TimeProblem::updateMultistepRhs: call updateSolutionMultiPreviousStep first");
        TEUCHOS_TEST_FOR_EXCEPTION(nmbToUse < 1 || nmbToUse > pendSteps_ || (int)coeff.size() < nmbToUse, std::logic_error,
                                   "TimeProblem::updateMultistepRhs: more coefficients asked for than steps recorded or coefficients given");
        pendMs_ = false;
        combineSystems();                                   // the merged time system: the history is as long as it
        std::vector<double> x = flatSolution();
        feddCheck(fedd_solution_set(dev_->ctx, x.data()), "fedd_solution_set");     // fedd_block_merge has reset it
        if (!msBegan_) {
            feddCheck(fedd_multistep_begin(dev_->ctx, pendSteps_), "fedd_multistep_begin");
            msBegan_ = true;
        }
        feddCheck(fedd_multistep_advance(dev_->ctx, SLOT_NL_MASS, nmbToUse, coeff.data()), "fedd_multistep_advance");
        feddCheck(fedd_rhs_get(dev_->ctx, x.data()), "fedd_rhs_get");
        size_t off = 0;
        auto rhs = problem_->getRhs();
        for (UN b = 0; b < rhs->size(); ++b) {
            auto& r = rhs->getBlockNonConst(b)->raw();
            std::copy(x.begin() + off, x.begin() + off + r.size(), r.begin());
            off += r.size();
        }
    }
    // the nonlinear problem's own entries on the time system: NavierStokes::reAssemble adds the advection to slot 6, so its
    // merged system IS (cm M + ca A + rho (N | N + W), B^T; B, C) and its residual b - S x (one fedd_spmv) already holds the
    // mass term the reference adds afterwards (:693-738, up to rounding); Dirichlet rows through setBCMinusVector / setVectorMinusBC
    void assemble(std::string type) const { needNl("assemble"); nl_->assemble(type); }
    void reAssemble(std::string type) const { needNl("reAssemble"); nl_->reAssemble(type); }
    // NonLinElasticity: the first call of a step uploads the step's right-hand side and source and begins the device's Newton
    // state; every call is one pass for the time tangent and the force, the Dirichlet rows of the tangent (fedd_dirichlet_nodes
    // writes the right-hand side of its rows, so it comes before the residual: setBoundariesSystem then finds them set), and
    // fedd_newton_residual, whose norm calculateResidualNorm returns.  No vector comes back to the host.
    void calculateNonLinResidualVec(std::string type = "standard", double time = 0.) {
        needNl("calculateNonLinResidualVec");
        if (nle_) {
            TEUCHOS_TEST_FOR_EXCEPTION(type != "reverse", std::logic_error,
                                       "TimeProblem::calculateNonLinResidualVec: the \"reverse\" residual is built for NonLinElasticity (the Newton loop asks for it)");
            fedd_ctx* ctx = dev_->ctx;
            const double cm = massParameters_[0][0];
            if (!stepOpen_) {
                feddCheck(fedd_rhs_set(ctx, problem_->getRhs()->getBlock(0)->raw().data()), "fedd_rhs_set");
                feddCheck(fedd_solution_set(ctx, problem_->getSolution()->getBlock(0)->raw().data()), "fedd_solution_set");
                feddCheck(fedd_newton_begin(ctx), "fedd_newton_begin");
                if (problem_->hasRhsFunction())      // NonLinElasticity::calculateNonLinResidualVec adds the source again (:254-263)
                    feddCheck(fedd_newton_source_set(ctx, problem_->getSourceTerm()->getBlock(0)->raw().data()), "fedd_newton_source_set");
                stepOpen_ = true;
            }
            nle_->reAssembleTime(SLOT_MASS, cm);
            nl_->setBoundariesSystem();
            std::vector<int32_t> flags, mask;
            std::vector<double> values;
            problem_->getBCFactory()->dirichletFlagTable(0, time, flags, mask, values);
            feddCheck(fedd_newton_residual(ctx, SLOT_MASS, cm, (int)flags.size(), flags.data(), mask.data(), values.data(), &residualNorm_),
                      "fedd_newton_residual");
            return;
        }
        combineSystems();
        nl_->calculateNonLinResidualVec(type, time);
    }
    double calculateResidualNorm() const { needNl("calculateResidualNorm"); return nle_ ? residualNorm_ : nl_->calculateResidualNorm(); }
    void setBoundariesSystem() const {
        needNl("setBoundariesSystem");
        if (nle_) return;       // set with the tangent, before the residual took the right-hand side (see calculateNonLinResidualVec)
        nl_->setBoundariesSystem();
    }
    void setBoundariesRHS(double time = .0) const { needNl("setBoundariesRHS"); nl_->setBoundariesRHS(time); }
    int solveUpdate() { needNl("solveUpdate"); return nl_->solveUpdate(); }
    int solveAndUpdate(const std::string& criterion, double& criterionValue) {
        needNl("solveAndUpdate");
        if (!nle_) return nl_->solveAndUpdate(criterion, criterionValue);
        // Schwarz setup on the time tangent, GMRES on the device's vectors (zero initial guess: the unknown is the update), u_k += delta
        auto pl = problem_->getParameterList();
        const std::string method = pl->sublist("General").get("Preconditioner Method", "Monolithic");
        TEUCHOS_TEST_FOR_EXCEPTION(method != "Monolithic", std::logic_error,
                                   "TimeProblem: \"Preconditioner Method\" = \"" + method + "\" is not built for time problems (Monolithic is; "
                                   "Diagonal and Triangular are built for the steady Stokes and Navier-Stokes problems)");
        auto& belos = pl->sublist("ThyraSolver").sublist("Linear Solver Types").sublist("Belos");
        const std::string solverType = belos.get("Solver Type", "Block GMRES");
        TEUCHOS_TEST_FOR_EXCEPTION(solverType != "Block GMRES", std::logic_error,
                                   "Solver Type \"" + solverType + "\" is not built for the nonlinear Newmark loop (Block GMRES is)");
        auto& gm = belos.sublist("Solver Types").sublist(solverType);
        const double tol = gm.get("Convergence Tolerance", 1e-8);
        const int maxIt = gm.get("Maximum Iterations", 100), numBlocks = gm.get("Num Blocks", 100);
        const bool usePrec = std::string(pl->sublist("ThyraPreconditioner").get("Preconditioner Type", "FROSch")) != "None";
        fedd_ctx* ctx = dev_->ctx;
        if (usePrec) LinearSolver<SC, LO, GO, NO>::setupSchwarz(ctx, pl->sublist("ThyraPreconditioner"), *pl, false, problem_->getVerbose());
        int its = 0;
        feddCheck(fedd_gmres(ctx, nullptr, nullptr, tol, maxIt, numBlocks, usePrec ? 1 : 0, &its, &lastRelativeResidual_), "fedd_gmres");
        double normDelta = 0.;
        feddCheck(fedd_newton_update(ctx, 1.0, &normDelta), "fedd_newton_update");
        if (criterion == "Update") criterionValue = normDelta;
        return its;
    }
    // the end of a step's nonlinear solve: u_{n+1} and the held right-hand side go back where fedd_newmark_advance looks for
    // them, and the host copies the public getters and the exporter read are refreshed -- once per step
    void endNonLinearStep() {
        if (!nle_ || !stepOpen_) return;
        fedd_ctx* ctx = dev_->ctx;
        feddCheck(fedd_rhs_get(ctx, nl_->getResidualVector()->getBlockNonConst(0)->raw().data()), "fedd_rhs_get");
        feddCheck(fedd_newton_end(ctx), "fedd_newton_end");
        feddCheck(fedd_solution_get(ctx, problem_->getSolution()->getBlockNonConst(0)->raw().data()), "fedd_solution_get");
        stepOpen_ = false;
    }
    bool getVerbose() const { return problem_->getVerbose(); }
    BlockMultiVectorPtr_Type getRhs() const { return problem_->getRhs(); }
    ParameterListPtr_Type getParameterList() const { return problem_->getParameterList(); }
    void updateTime(double time) { time_ = time; }
    void assembleSourceTerm(double time) { problem_->assembleSourceTerm(time); }
    bool hasSourceTerm() const { return problem_->hasSourceTerm(); }
    BlockMultiVectorPtr_Type getSourceTerm() { return problem_->getSourceTerm(); }
    void addToRhs(BlockMultiVectorPtr_Type x) { problem_->addToRhs(x); }
    // a rebuilt matrix gets its Dirichlet rows and values (BCBuilder::set); while it stands only the values of the
    // right-hand side are set, so the preconditioner and the solver's SpMV setup stand too
    void setBoundaries(double time = .0) {
        auto bc = problem_->getBCFactory();
        TEUCHOS_TEST_FOR_EXCEPTION(bc.is_null(), std::runtime_error, "No boundary conditions added.");
        if (fresh_) bc->set(systemCombined_, problem_->getRhs(), time);
        else bc->setRHS(problem_->getRhs(), time);
    }
    // the existing LinearSolver on the combined matrix, the previous solution as the initial guess; the preconditioner is
    // built when the matrix was rebuilt and kept otherwise ("MonolithicConstPrec")
    int solve() {
        auto pl = problem_->getParameterList();
        const bool zeroGuess = pl->get("Zero Initial Guess", true);
        pl->set("Zero Initial Guess", false);
        BlockMatrixPtr_Type steady = problem_->system_;
        problem_->system_ = systemCombined_;
        LinearSolver<SC, LO, GO, NO> linSolver;
        int its = 0;
        const std::string method = pl->sublist("General").get("Preconditioner Method", "Monolithic");
        TEUCHOS_TEST_FOR_EXCEPTION(method != "Monolithic", std::logic_error,
                                   "TimeProblem: \"Preconditioner Method\" = \"" + method + "\" is not built for time problems (Monolithic is; "
                                   "Diagonal and Triangular are built for the steady Stokes and Navier-Stokes problems)");
        try {
            its = linSolver.solve(problem_, Teuchos::null, fresh_ ? "Monolithic" : "MonolithicConstPrec");
        } catch (...) {
            problem_->system_ = steady;
            pl->set("Zero Initial Guess", zeroGuess);
            throw;
        }
        problem_->system_ = steady;
        pl->set("Zero Initial Guess", zeroGuess);
        fresh_ = false;
        lastRelativeResidual_ = linSolver.lastRelativeResidual;
        if (problem_->getVerbose()) std::cout << "-- time " << time_ << ": " << its << " iterations, relative residual " << lastRelativeResidual_ << std::endl;
        return its;
    }
    BlockMultiVectorPtr_Type getSolution() { return problem_->getSolution(); }
    BlockMatrixPtr_Type getSystemCombined() const { return systemCombined_; }
    BlockMatrixPtr_Type getMassSystem() const { return systemMass_; }
    Problem_Type* getUnderlyingProblem() { return problem_; }
    double getLastRelativeResidual() const { return lastRelativeResidual_; }
    int numberOfCombines() const { return combines_; }
private:
    void needNl(const char* who) const {
        TEUCHOS_TEST_FOR_EXCEPTION(!nl_, std::logic_error, std::string("TimeProblem::") + who + ": the wrapped problem is linear");
    }
    std::vector<double> flatSolution() const {
        std::vector<double> x;
        auto sol = problem_->getSolution();
        for (UN b = 0; b < sol->size(); ++b) x.insert(x.end(), sol->getBlock(b)->raw().begin(), sol->getBlock(b)->raw().end());
        return x;
    }
    Problem_Type* problem_;
    NonLinearProblem_Type* nl_ = nullptr;
    NavierStokes_Type* ns_ = nullptr;
    NonLinElasticity_Type* nle_ = nullptr;
    bool stepOpen_ = false;
    double residualNorm_ = 0.;
    bool nlCombined_ = false, msBegan_ = false, pendMs_ = false;
    double nlCm_ = 0., nlCa_ = 0.;
    int pendSteps_ = 0;
    CommConstPtr_Type comm_;
    DeviceContextPtr dev_;
    SmallMatrix<int> timeStepDef_;
    SmallMatrix<double> massParameters_, timeParameters_;
    BlockMatrixPtr_Type systemMass_, systemCombined_;
    bool fresh_ = false, began_ = false, pend_ = false;
    double pendDt_ = 0., pendBeta_ = 0., pendGamma_ = 0., time_ = 0., lastRelativeResidual_ = 0.;
    int combines_ = 0;
};

// NonLinearSolver::solve(TimeProblem&, time): the TimeProblem overloads of the reference's fixed-point and Newton loops
// (NonLinearSolver_def.hpp:394-452, 459-531), line by line
template <class SC, class LO, class GO, class NO>
void NonLinearSolver<SC, LO, GO, NO>::solve(TimeProblem_Type& problem, double time) {
    TEUCHOS_TEST_FOR_EXCEPTION(type_ != "FixedPoint" && type_ != "Newton", std::logic_error,
                               "\"Linearization\" = \"" + type_ + "\" is not built for time problems (FixedPoint and Newton are; Extrapolation and NOX are not)");
    TEUCHOS_TEST_FOR_EXCEPTION(!problem.isNonLinear(), std::logic_error, "NonLinearSolver: the time problem wraps a linear problem");
    const bool newton = type_ == "Newton";
    // NonLinElasticity::reAssembleExtrapolation (NonLinElasticity_def.hpp:129-134), which the fixed-point loop would reach
    TEUCHOS_TEST_FOR_EXCEPTION(!newton && problem.isNonLinElasticity(), std::logic_error,
                               "Only Newton implemented for nonlinear material models! (\"Linearization\" = \"" + type_ + "\" on NonLinElasticity; Newton is built)");
    const bool verbose = problem.getVerbose();
    problem.setBoundariesRHS(time);
    TEUCHOS_TEST_FOR_EXCEPTION(problem.getRhs()->getNumVectors() != 1, std::logic_error, "We need to change the code for numVectors>1.");
    const char* name = newton ? "Newton" : "Fixed Point";
    double gmresIts = 0., residual0 = 1., residual = 1.;
    auto& par = problem.getParameterList()->sublist("Parameter");
    const double tol = par.get("relNonLinTol", 1.0e-6);
    int nlIts = 0;
    const int maxNonLinIts = par.get("MaxNonLinIts", 10);
    double criterionValue = 1.;
    const std::string criterion = par.get("Criterion", "Residual");
    while (nlIts < maxNonLinIts) {
        problem.calculateNonLinResidualVec("reverse", time);
        if (criterion == "Residual") residual = problem.calculateResidualNorm();
        if (nlIts == 0) residual0 = residual;
        if (!newton) {                      // :423-427: the linearised matrix is combined with the mass matrix, then the boundary rows
            problem.combineSystems();
            problem.setBoundariesSystem();
        }
        if (criterion == "Residual") {
            criterionValue = residual / residual0;
            if (verbose) std::cout << "### " << name << " iteration : " << nlIts << "  relative nonlinear residual : " << criterionValue << std::endl;
            if (criterionValue < tol) break;
        }
        if (newton) {                       // :495-498
            problem.assemble("Newton");
            problem.setBoundariesSystem();
        }
        gmresIts += problem.solveAndUpdate(criterion, criterionValue);
        nlIts++;
        if (criterion == "Update") {
            if (verbose) std::cout << "### " << name << " iteration : " << nlIts << "  residual of update : " << criterionValue << std::endl;
            if (criterionValue < tol) break;
        }
    }
    gmresIts /= std::max(nlIts, 1);
    lastNonLinIts = nlIts;
    if (verbose)
        std::cout << "### Total " << (newton ? "Newton iteration" : "FPI") << " : " << nlIts << "  with average gmres its : " << gmresIts << std::endl;
    if (par.get("Cancel MaxNonLinIts", false))
        TEUCHOS_TEST_FOR_EXCEPTION(nlIts == maxNonLinIts, std::runtime_error,
                                   "Maximum nonlinear Iterations reached. Problem might have converged in the last step. Still we cancel here.");
}

template <class SC = default_sc, class LO = default_lo, class GO = default_go, class NO = default_no>
class DAESolverInTime {
public:
    typedef Problem<SC, LO, GO, NO> Problem_Type;
    typedef TimeProblem<SC, LO, GO, NO> TimeProblem_Type;
    typedef Teuchos::RCP<const Teuchos::Comm<int>> CommConstPtr_Type;
    typedef ExporterParaView<SC, LO, GO, NO> Exporter_Type;

    DAESolverInTime(ParameterListPtr_Type& parameterList, CommConstPtr_Type comm) : parameterList_(parameterList), comm_(comm) {}
    void defineTimeStepping(const SmallMatrix<int>& def) { timeStepDef_ = def; }
    void setProblem(Problem_Type& problem) {
        problem_ = &problem;
        nonLinear_ = dynamic_cast<NonLinearProblem<SC, LO, GO, NO>*>(&problem) != nullptr;
        problemTime_.reset(new TimeProblem_Type(problem, comm_));
    }
    void setupTimeStepping() {                                          // DAESolverInTime_def.hpp: setupTimeStepping
        TEUCHOS_TEST_FOR_EXCEPTION(problemTime_.is_null(), std::logic_error, "DAESolverInTime: call setProblem first");
        checkClass();
        ParameterListPtr_Type tsl(new Teuchos::ParameterList(parameterList_->sublist("Timestepping Parameter")));
        timeSteppingTool_.reset(new TimeSteppingTools(tsl, comm_));
        problemTime_->setTimeDef(timeStepDef_);
        problemTime_->assembleMassSystem();
    }
    void advanceInTime() {
        TEUCHOS_TEST_FOR_EXCEPTION(timeSteppingTool_.is_null(), std::logic_error, "DAESolverInTime: call setupTimeStepping first");
        checkClass();
        if (nonLinear_ && problemTime_->isNonLinElasticity()) advanceInTimeNonLinearNewmark();
        else if (nonLinear_) advanceInTimeNonLinearMultistep();
        else advanceInTimeLinearNewmark();
    }
    const std::vector<int>& nonLinearIterations() const { return nlItsPerStep_; }
    Teuchos::RCP<TimeProblem_Type> getTimeProblem() const { return problemTime_; }
    int stepsDone() const { return timeSteppingTool_.is_null() ? 0 : timeSteppingTool_->currentStep(); }
private:
    void checkClass() const {
        // "Newmark" + linear and "Multistep" + nonlinear are built; the reference's default class is "Singlestep"
        const std::string cls = parameterList_->sublist("Timestepping Parameter").get("Class", nonLinear_ ? "Singlestep" : "Newmark");
        const bool nle = !problemTime_.is_null() && problemTime_->isNonLinElasticity();
        const bool ok = nonLinear_ ? (nle ? cls == "Newmark" : cls == "Multistep") : cls == "Newmark";
        TEUCHOS_TEST_FOR_EXCEPTION(!ok, std::logic_error,
                                   "Timestepping Parameter \"Class\" = \"" + cls + "\" on " + (nle ? "NonLinElasticity" : nonLinear_ ? "a nonlinear problem" : "a linear problem") +
                                       " is not built (Singlestep and External are not); \"Newmark\" on a linear problem and on NonLinElasticity "
                                       "(1 x 1 time definition, Newton) and \"Multistep\" (BDF 1, 2) on NavierStokes are");
        if (nonLinear_) {
            const std::string lin = parameterList_->sublist("General").get("Linearization", "FixedPoint");
            TEUCHOS_TEST_FOR_EXCEPTION(nle && lin == "FixedPoint", std::logic_error,
                                       "Only Newton implemented for nonlinear material models! (\"Linearization\" = \"FixedPoint\" on NonLinElasticity; Newton is built)");
            TEUCHOS_TEST_FOR_EXCEPTION(nle && timeStepDef_.size() != 1, std::logic_error,
                                       "Newmark only implemented for systems of size 1x1: NonLinElasticity takes the 1 x 1 time definition [[1]] (\"Newmark\", Newton), a " +
                                           std::to_string(timeStepDef_.size()) + " x " + std::to_string(timeStepDef_.size()) + " definition was given");
            TEUCHOS_TEST_FOR_EXCEPTION(lin != "FixedPoint" && lin != "Newton", std::logic_error,
                                       "\"Linearization\" = \"" + lin + "\" is not built for time problems (FixedPoint and Newton are; Extrapolation and NOX are not)");
        }
    }
    // DAESolverInTime::advanceInTimeNonLinearMultistep (:1209-1333), in the reference's order
    void advanceInTimeNonLinearMultistep() {
        const bool print = parameterList_->sublist("General").get("ParaViewExport", false);
        if (print) exportTimestep();
        const int size = timeStepDef_.size();
        const double dt = timeSteppingTool_->get_dt();
        const int nmbBDF = timeSteppingTool_->getBDFNumber();
        vec_dbl_Type coeffPrevSteps((size_t)nmbBDF);
        for (int i = 0; i < nmbBDF; ++i) coeffPrevSteps[(size_t)i] = timeSteppingTool_->getInformationBDF(i + 2) / dt;
        SmallMatrix<double> massCoeff(size), problemCoeff(size);
        for (int i = 0; i < size; ++i)
            for (int j = 0; j < size; ++j) {
                massCoeff[i][j] = (timeStepDef_[i][j] > 0 && i == j) ? timeSteppingTool_->getInformationBDF(0) / dt : 0.;
                problemCoeff[i][j] = timeStepDef_[i][j] > 0 ? timeSteppingTool_->getInformationBDF(1) : 1.;
            }
        problemTime_->setTimeParameters(massCoeff, problemCoeff);
        const std::string linearization = parameterList_->sublist("General").get("Linearization", "FixedPoint");
        while (timeSteppingTool_->continueTimeStepping()) {
            const bool firstStep = timeSteppingTool_->currentTime() == 0.;
            if (firstStep) {                                            // BDF1 for the first time step
                SmallMatrix<double> tmpMassCoeff(size), tmpProblemCoeff(size);
                for (int i = 0; i < size; ++i)
                    for (int j = 0; j < size; ++j) {
                        tmpMassCoeff[i][j] = (timeStepDef_[i][j] > 0 && i == j) ? 1. / dt : 0.;
                        tmpProblemCoeff[i][j] = 1.;
                    }
                problemTime_->setTimeParameters(tmpMassCoeff, tmpProblemCoeff);
            }
            problemTime_->updateSolutionMultiPreviousStep(nmbBDF);
            const double time = timeSteppingTool_->currentTime() + dt;
            problemTime_->updateTime(time);
            if (firstStep) {
                vec_dbl_Type tmpCoeffPrevSteps(1, 1. / dt);
                problemTime_->updateMultistepRhs(tmpCoeffPrevSteps, 1);
            } else {
                problemTime_->updateMultistepRhs(coeffPrevSteps, nmbBDF);
            }
            // :1303-1304; the source vector of this facade exists from initializeProblem on, so the question is whether a function fills it
            TEUCHOS_TEST_FOR_EXCEPTION(problem_->hasRhsFunction(), std::logic_error, "Check sourceterm.");
            NonLinearSolver<SC, LO, GO, NO> nlSolver(linearization);
            nlSolver.solve(*problemTime_, time);
            nlItsPerStep_.push_back(nlSolver.lastNonLinIts);
            if (firstStep) problemTime_->setTimeParameters(massCoeff, problemCoeff);   // the desired BDF parameters from now on
            timeSteppingTool_->advanceTime(true);
            if (print) exportTimestep();
        }
        comm_->barrier();
        if (print && !exporter_.is_null()) exporter_->closeExporter();
        if (print && !exporterP_.is_null()) exporterP_->closeExporter();
    }
    // DAESolverInTime::advanceInTimeLinearNewmark (:519-607), in the reference's order
    void advanceInTimeLinearNewmark() {
        const bool print = parameterList_->sublist("General").get("ParaViewExport", false);
        if (print) exportTimestep();
        TEUCHOS_TEST_FOR_EXCEPTION(timeStepDef_.size() > 1, std::runtime_error, "Newmark only implemented for systems of size 1x1.");
        const double dt = timeSteppingTool_->get_dt(), beta = timeSteppingTool_->get_beta(), gamma = timeSteppingTool_->get_gamma();
        SmallMatrix<double> massCoeff(1), problemCoeff(1);
        massCoeff[0][0] = 1.0 / (dt * dt * beta);
        problemCoeff[0][0] = 1.0;
        const double coeffSourceTerm = 1.0;
        vec_dbl_Type coeffTemp(1, 1.0);
        problemTime_->setTimeParameters(massCoeff, problemCoeff);
        while (timeSteppingTool_->continueTimeStepping()) {
            problemTime_->combineSystems();
            problemTime_->updateSolutionNewmarkPreviousStep(dt, beta, gamma);
            const double time = timeSteppingTool_->currentTime() + dt;
            problemTime_->updateTime(timeSteppingTool_->currentTime());
            problemTime_->updateNewmarkRhs(dt, beta, gamma, coeffTemp);
            if (problemTime_->hasSourceTerm()) {
                problemTime_->assembleSourceTerm(time);
                addSourceTermToRHS(coeffSourceTerm);
            }
            problemTime_->setBoundaries(time);
            problemTime_->solve();
            timeSteppingTool_->advanceTime(true);
            if (print) exportTimestep();
        }
        comm_->barrier();
        if (print && !exporter_.is_null()) exporter_->closeExporter();
    }
    // DAESolverInTime::advanceInTimeNonLinearNewmark (:613-722), in the reference's order
    void advanceInTimeNonLinearNewmark() {
        const bool print = parameterList_->sublist("General").get("ParaViewExport", false);
        if (print) exportTimestep();
        TEUCHOS_TEST_FOR_EXCEPTION(timeStepDef_.size() > 1, std::runtime_error, "Newmark only implemented for systems of size 1x1.");
        const double dt = timeSteppingTool_->get_dt(), beta = timeSteppingTool_->get_beta(), gamma = timeSteppingTool_->get_gamma();
        SmallMatrix<double> massCoeff(1), problemCoeff(1);
        massCoeff[0][0] = 1.0 / (dt * dt * beta);
        problemCoeff[0][0] = 1.0;
        const double coeffSourceTerm = 1.0;
        vec_dbl_Type coeffTemp(1, 1.0);
        problemTime_->setTimeParameters(massCoeff, problemCoeff);
        const std::string linearization = parameterList_->sublist("General").get("Linearization", "FixedPoint");
        while (timeSteppingTool_->continueTimeStepping()) {
            problemTime_->combineSystems();
            problemTime_->updateSolutionNewmarkPreviousStep(dt, beta, gamma);
            const double time = timeSteppingTool_->currentTime() + dt;
            problemTime_->updateTime(time);
            problemTime_->updateNewmarkRhs(dt, beta, gamma, coeffTemp);
            if (problemTime_->hasSourceTerm()) {
                problemTime_->assembleSourceTerm(time);
                addSourceTermToRHS(coeffSourceTerm);
            }
            NonLinearSolver<SC, LO, GO, NO> nlSolver(linearization);
            try {
                nlSolver.solve(*problemTime_, time);
            } catch (...) {
                problemTime_->endNonLinearStep();
                throw;
            }
            problemTime_->endNonLinearStep();
            nlItsPerStep_.push_back(nlSolver.lastNonLinIts);
            timeSteppingTool_->advanceTime(true);
            if (print) exportTimestep();
        }
        comm_->barrier();
        if (print && !exporter_.is_null()) exporter_->closeExporter();
    }
    void addSourceTermToRHS(double coeff) {                            // :1444-1450
        auto rhs = problemTime_->getUnderlyingProblem()->getRhs();
        rhs->update(coeff, *problemTime_->getSourceTerm(), 1.);
    }
    void exportTimestep() {
        if (exporter_.is_null()) {
            exporter_.reset(new Exporter_Type());
            auto dom = problem_->getDomain(0);
            exporter_->setup(problem_->getVariableName(0), dom->getMesh(), problem_->getFEType(0));
            exportSolution_ = problem_->getSolution()->getBlock(0);
            const int dofs = problem_->getDofsPerNode(0);
            exporter_->addVariable(exportSolution_, problem_->getVariableName(0), dofs > 1 ? "Vector" : "Scalar", dofs, dom->getMapUnique());
            if (nonLinear_ && problem_->getSolution()->size() > 1) {    // velocity and pressure per step
                exporterP_.reset(new Exporter_Type());
                auto domP = problem_->getDomain(1);
                exporterP_->setup(problem_->getVariableName(1), domP->getMesh(), problem_->getFEType(1));
                exportSolutionP_ = problem_->getSolution()->getBlock(1);
                exporterP_->addVariable(exportSolutionP_, problem_->getVariableName(1), "Scalar", 1, domP->getMapUnique());
            }
        }
        exporter_->save(timeSteppingTool_->currentTime());
        if (!exporterP_.is_null()) exporterP_->save(timeSteppingTool_->currentTime());
    }
    ParameterListPtr_Type parameterList_;
    CommConstPtr_Type comm_;
    SmallMatrix<int> timeStepDef_;
    Problem_Type* problem_ = nullptr;
    Teuchos::RCP<TimeProblem_Type> problemTime_;
    Teuchos::RCP<TimeSteppingTools> timeSteppingTool_;
    Teuchos::RCP<Exporter_Type> exporter_, exporterP_;
    Teuchos::RCP<const MultiVector<SC, LO, GO, NO>> exportSolution_, exportSolutionP_;
    bool nonLinear_ = false;
    std::vector<int> nlItsPerStep_;
};

}  // namespace FEDD
